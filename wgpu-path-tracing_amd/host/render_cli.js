#!/usr/bin/env node
'use strict';
/**
 * render_cli.js — drives the Renderer the way the reference's frame loop does
 * (renderer.ts:415-454: one dispatch per frame, frameIndex++), headless:
 *   node render_cli.js <scene.ptscene> <out.f32> [--width W --height H --frames N --bounces B --mis 0|1
 *                       --aperture A --focus F --batch K --png out.png --denoise
 *                       --adaptive THRESHOLD --max-frames N --rounds R
 *                       --env file.hdr --env-intensity X --env-rotation DEGREES --env-sample 0|1
 *                       --fog sigma_t[,albedo[,g]] --fog-density file.f32 --fog-grid nx,ny,nz --fog-filter nearest|linear
 *                       --devices 0,1,... --loopback --aov albedo|normal|id --aov-out plane.bin
 *                       --alpha-cutout --alpha-blend --alpha-seed N --alpha-layers N --animation N --time S
 *                       --camera N --projection ortho|panorama --ymag V --hdr out.hdr
 *                       --bake W,H --bake-dilate N --bake-bias B --bake-denoise --bake-denoise-iterations N
 *                       --probes nx,ny,nz --probe-tile N --probe-irradiance M
 *                       --probe-visibility M [--probe-sharpness S] [--probe-max-distance D] [--probe-border]]
 * --batch K traces K frames per dispatch instead of one. --denoise keeps the denoiser's planes and makes --png the tone-mapped
 * denoised image (include/ptmi.h ptmi_denoise, default parameters). --adaptive renders to a noise level instead of --frames
 * (include/ptmi.h ptmi_dispatch_adaptive): rounds until none lists a pixel, or --rounds R of them; the JSON line then also holds
 * adaptive: { samples, minCount, maxCount, rounds }. --env lights the scene with a Radiance .hdr environment map (hdr_decode.js;
 * include/ptmi.h ptmi_upload_environment): equirectangular, scaled by --env-intensity, turned by --env-rotation degrees about +Y;
 * --env-sample 1 only looks it up. --fog fills the scene's box with a homogeneous scattering medium (include/ptmi.h ptmi_set_medium):
 * extinction sigma_t per unit length, single-scattering albedo (default 1) and Henyey-Greenstein asymmetry g (default 0); --fog-density gives it a density grid
 * (ptmi_upload_medium_density): a raw file of nx * ny * nz float32 values, x fastest, looked up per cell or with --fog-filter linear. Values in [0, 1]
 * are taken as they are, as multipliers of sigma_t; a file that holds larger ones is divided by its maximum (sigma_t is then the
 * extinction at its densest cell). Writes W*H*4 float32 (the output buffer, raw also with
 * --denoise) and prints one JSON line with the statistics. --devices renders on several GPUs behind one Renderer (include/ptmi.h
 * ptmi_multi_*; --loopback lets one ordinal be listed more than once, for a one-GPU box); --adaptive, --denoise and --aov work with
 * it. --aov keeps that first-hit plane and --aov-out writes it raw (float32 x 4 per pixel, uint32 x 2 for id).
 * --alpha-cutout (a .glb scene): materials with alphaMode "MASK" become cutouts at their alphaCutoff (include/ptmi.h
 * ptmi_set_alpha_cutoff): the atlas keeps the alpha of albedo maps, and paths and shadow rays pass where it is below the cutoff, through
 * at most --alpha-layers N holes per segment (default: the library's, 4); the JSON line then also holds alpha: the table's status.
 * --alpha-blend (a .glb scene): materials with alphaMode "BLEND" are blended with their baseColorFactor[3] as hashed stochastic
 * transparency (include/ptmi.h ptmi_set_alpha_blend; --alpha-seed N: the hash's seed, --alpha-layers as above); the JSON line then
 * also holds alphaBlend: the table's status.
 * --animation N --time S (a .glb scene with a skin or morph targets): renders one frame posed at S seconds (default 0) of the file's
 * animation N (Renderer.poseAt; include/ptmi.h ptmi_pose_morph, ptmi_pose_skin); the JSON line then also holds skin and morph: their
 * status.
 * --camera N (a .glb scene) looks through the file's camera N (Renderer.useSceneCamera: position, basis, yfov or ymag, projection; the
 * frame keeps --width x --height, so the file's vertical extent is kept and its aspect ratio is not). --projection ortho renders
 * orthographically with the half-height --ymag V in world units (default 1); --projection panorama renders the full sphere about the
 * camera position as an equirectangular image (include/ptmi.h ptmi_set_projections), best with a 2:1 frame. --hdr out.hdr also writes
 * the output buffer as a Radiance file, top row first; for a panorama it is laid out as an environment map (hdr_encode.js), so that
 * --env out.hdr lights another scene with what this camera saw. The JSON line then also holds projection.
 * --bake W,H bakes a W x H lightmap instead of rendering from the camera (Renderer.bake; include/ptmi.h ptmi_dispatch_bake): --frames
 * samples per covered texel over the scene's lightmap coordinates (a .glb's TEXCOORD_1, else TEXCOORD_0), --bake-dilate N gutter-fill
 * passes (default 0), --bake-bias B the origin offset along the first ray (default 1e-6). out.f32 and --hdr then hold the lightmap
 * (row y at v = (y + 0.5) / H; w: 0, or with --bake-dilate the texel's state), --png its tone-mapped image, and the JSON line bake:
 * { width, height, frames, covered }. --bake-denoise filters the lightmap over the bake surface before the gutter fill (include/ptmi.h
 * ptmi_bake_denoise, default parameters; --bake-denoise-iterations N passes, default 5): w is then the texel's state, and bake also
 * holds denoised: true. Not with --devices, --denoise, --aov or --adaptive.
 * --probes nx,ny,nz gathers light probes instead of rendering from the camera (Renderer.bakeProbes; include/ptmi.h
 * ptmi_dispatch_probes): an nx x ny x nz lattice over the scene's bounds with a probe at every cell centre (probes.js grid), so the
 * outermost probes stand half a cell inside the bounds; --probe-tile N the atlas tile (default 8), --frames samples per atlas texel,
 * --probe-irradiance M also the M x M irradiance tiles. out.f32 then holds the radiance atlas (its size in the JSON line's probes:
 * { width, height, count, tile }), and beside it <out minus .f32>.sh.f32 holds 27 floats per probe and, with --probe-irradiance,
 * <out minus .f32>.irr.f32 the M * M float4 per probe. Not with --devices, --denoise, --aov, --adaptive or --bake.
 * --probe-visibility M also gathers the probes' depth and writes <out minus .f32>.vis.f32, the M x M visibility tiles (mean distance,
 * mean squared distance, hit fraction, 1; include/ptmi.h ptmi_probe_visibility): --probe-sharpness S the log2 of the lobe's exponent
 * (default 6), --probe-max-distance D the clamp (default 1.5 cell diagonals of the lattice), --probe-border a ring of wrapped texels
 * for bilinear taps around every visibility tile and every irradiance tile of out.irr.f32: (M + 2)^2 float4 per probe.
 */
var fs = require('fs');
var host = require('./renderer');

function arg(name, dflt) {
  var i = process.argv.indexOf('--' + name);
  return i >= 0 ? Number(process.argv[i + 1]) : dflt;
}

var scenePath = process.argv[2], outPath = process.argv[3];
if (!scenePath || !outPath) { console.error('usage: render_cli.js scene.ptscene out.f32 [options]'); process.exit(2); }
var W = arg('width', 256), H = arg('height', 256), frames = arg('frames', 16), batch = arg('batch', 1);
var denoise = process.argv.indexOf('--denoise') >= 0;
var adaptive = process.argv.indexOf('--adaptive') >= 0 ? { threshold: arg('adaptive', 0), maxFrames: arg('max-frames', 0) } : null;

function textArg(name) {
  var i = process.argv.indexOf('--' + name);
  return i >= 0 ? process.argv[i + 1] : null;
}
var devices = textArg('devices') ? textArg('devices').split(',').map(Number) : null;
var aov = textArg('aov');

var alphaCutout = process.argv.indexOf('--alpha-cutout') >= 0, alphaBlend = process.argv.indexOf('--alpha-blend') >= 0;
var r = new host.Renderer({ width: W, height: H, devices: devices || undefined, loopback: process.argv.indexOf('--loopback') >= 0,
                            alphaCutout: alphaCutout, alphaLayers: arg('alpha-layers', 0),
                            alphaBlend: alphaBlend, alphaBlendSeed: arg('alpha-seed', 0),
                            projections: textArg('camera') !== null || textArg('projection') !== null,
                            options: { maxBounces: arg('bounces', 8), doMis: arg('mis', 1) } });
r.camera.aperture = arg('aperture', r.camera.aperture);
r.camera.focusDistance = arg('focus', r.camera.focusDistance);
if (denoise) r.setDenoise(true);
if (aov) {                                 // beside the denoiser's planes, when those are on
  var names = denoise ? ['normal', 'albedo'] : [];
  if (names.indexOf(aov) < 0) names.push(aov);
  r.setAovs(names);
}
var envAt = process.argv.indexOf('--env');
r.loadModel(scenePath).then(function () {
  if (envAt >= 0) {
    var env = require('./hdr_decode').decodeHDR(fs.readFileSync(process.argv[envAt + 1]));
    r.setEnvironment(env.data, env.width, env.height,
                     { intensity: arg('env-intensity', 1), rotation: arg('env-rotation', 0) * Math.PI / 180, sample: arg('env-sample', 0) });
  }
  if (textArg('fog')) {
    var fog = textArg('fog').split(',').map(Number);
    r.setMedium({ sigmaT: fog[0], albedo: fog.length > 1 ? fog[1] : 1, g: fog.length > 2 ? fog[2] : 0, bounds: 'scene' });
  }
  if (textArg('fog-density')) {
    if (!textArg('fog') || !textArg('fog-grid')) throw new Error('--fog-density needs --fog and --fog-grid nx,ny,nz');
    var dims = textArg('fog-grid').split(',').map(Number);
    var raw = fs.readFileSync(textArg('fog-density'));
    if (dims.length !== 3 || raw.length !== dims[0] * dims[1] * dims[2] * 4) throw new Error('--fog-density: the file is not nx * ny * nz float32 values');
    var rho = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length));
    var peak = 0;
    for (var k = 0; k < rho.length; k++) peak = Math.max(peak, rho[k]);
    // multipliers in [0, 1] are taken as they are; larger densities are divided by their maximum, with sigma_t left as given: the file
    // then says where the fog is, --fog how thick it is at its thickest
    if (peak > 1) for (var q = 0; q < rho.length; q++) rho[q] /= peak;
    r.setMediumDensity(rho, dims, { filter: textArg('fog-filter') || 'nearest' });
  }
  if (textArg('animation') !== null) r.poseAt(arg('animation', 0), arg('time', 0));
  if (textArg('camera') !== null) r.useSceneCamera(arg('camera', 0));
  var projection = textArg('projection');
  if (projection !== null) {
    if (projection !== 'ortho' && projection !== 'panorama') throw new Error('--projection: ortho or panorama, not ' + projection);
    r.setProjection(projection === 'ortho' ? 'orthographic' : 'equirect', { ymag: arg('ymag', r.camera.ymag || 1) });
  } else if (textArg('ymag') !== null && r.camera.projection === 'orthographic') r.setProjection('orthographic', { ymag: arg('ymag', 1) });
  var t0 = Date.now();
  var status = null, out = null, probeSet = null;
  if (textArg('bake') !== null) {
    var size = textArg('bake').split(',').map(Number);
    if (size.length !== 2 || !(size[0] > 0) || !(size[1] > 0)) throw new Error('--bake: W,H');
    if (devices || denoise || aov || adaptive) throw new Error('--bake does not go with --devices, --denoise, --aov or --adaptive');
    out = r.bake({ width: size[0], height: size[1], frames: frames, dilate: arg('bake-dilate', 0), bias: arg('bake-bias', 1e-6),
      denoise: process.argv.indexOf('--bake-denoise') >= 0 ? { iterations: arg('bake-denoise-iterations', 0) } : false });
    W = size[0]; H = size[1];
  } else if (textArg('probes') !== null) {
    var counts = textArg('probes').split(',').map(Number);
    if (counts.length !== 3 || !(counts[0] > 0) || !(counts[1] > 0) || !(counts[2] > 0)) throw new Error('--probes: nx,ny,nz');
    if (devices || denoise || aov || adaptive) throw new Error('--probes does not go with --devices, --denoise, --aov or --adaptive');
    if (!r.sceneBounds) throw new Error('--probes needs a scene with a hierarchy (its bounds)');
    var stem = outPath.replace(/\.f32$/, '');
    var visTile = arg('probe-visibility', 0);
    probeSet = r.bakeProbes({ grid: { min: r.sceneBounds.min, max: r.sceneBounds.max, counts: counts }, tile: arg('probe-tile', 8),
                              frames: frames, irradiance: arg('probe-irradiance', 0),
                              visibility: visTile ? { tile: visTile, sharpness: arg('probe-sharpness', 6), maxDistance: arg('probe-max-distance', 0),
                                                      border: process.argv.indexOf('--probe-border') >= 0 } : null });
    out = probeSet.radiance; W = probeSet.width; H = probeSet.height;
    fs.writeFileSync(stem + '.sh.f32', Buffer.from(probeSet.sh.buffer));
    if (probeSet.irradiance) fs.writeFileSync(stem + '.irr.f32', Buffer.from(probeSet.irradiance.buffer));
    if (probeSet.visibility) fs.writeFileSync(stem + '.vis.f32', Buffer.from(probeSet.visibility.buffer));
  } else if (adaptive) {
    r.setAdaptive(adaptive);
    var rounds = arg('rounds', 0);
    if (rounds > 0) r.renderAdaptive(rounds);
    else do { r.renderAdaptive(1); } while (r.adaptiveStatus().active > 0);
    status = r.adaptiveStatus();
  } else
    while (r.frameIndex < frames) r.renderFrame(Math.min(batch, frames - r.frameIndex));
  if (!out) out = r.readOutput();
  var ms = Date.now() - t0;
  fs.writeFileSync(outPath, Buffer.from(out.buffer));
  if (aov && textArg('aov-out')) { var plane = r.readAov(aov); fs.writeFileSync(textArg('aov-out'), Buffer.from(plane.buffer)); }
  if (textArg('hdr')) {
    var enc = require('./hdr_encode'), top = new Float32Array(out.length);
    if (r.camera.projection === 'equirect') top = enc.panoramaToEnvironment(out, W, H);
    else for (var row = 0; row < H; row++) top.set(out.subarray((H - 1 - row) * W * 4, (H - row) * W * 4), row * W * 4);
    fs.writeFileSync(textArg('hdr'), enc.encodeHDR(top, W, H));
  }
  var pi = process.argv.indexOf('--png');
  if (pi >= 0) {
    var img;
    if (denoise) { r.denoise(); img = r.blitDenoised(); } else img = r.blit();
    fs.writeFileSync(process.argv[pi + 1], require('./png').encodePNG(img, W, H));
  }
  var st = r.getStats();
  st.wallMs = ms; st.width = W; st.height = H; st.frames = frames;
  if (status) st.frames = 0;                // no uniform frames: the counts are per pixel
  if (alphaCutout) st.alpha = r.alphaStatus();
  if (alphaBlend) st.alphaBlend = r.alphaBlendStatus();
  if (textArg('animation') !== null) { st.skin = r.skinStatus(); st.morph = r.morphStatus(); }
  if (r.projections) st.projection = { kind: r.camera.projection || 'perspective', ymag: r.camera.ymag || 0 };
  if (r.lastBake) st.bake = r.lastBake;
  if (probeSet) st.probes = { width: W, height: H, count: probeSet.count, tile: arg('probe-tile', 8) };
  if (status) st.adaptive = { samples: status.samples, minCount: status.minCount, maxCount: status.maxCount, rounds: status.rounds };
  console.log(JSON.stringify(st));
  r.destroy();
}).catch(function (e) { console.error(String(e && e.stack || e)); process.exit(1); });
