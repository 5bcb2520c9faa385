'use strict';
/**
 * renderer.js — Node host with the reference Renderer's public surface
 * (src/renderer/renderer.ts:18-511: loadModel, start, stop, destroy, resize, moveCamera,
 * rotateCamera, addOnUpdate, camera) whose compute pass runs on the MI355X through the
 * N-API addon instead of WebGPU:
 *
 *   createBuffers + createBindGroups (renderer.ts:242-355, :368-381) -> uploadScene / uploadAtlas / resize
 *   updateCamera                      (renderer.ts:403-413)          -> packCamera (96-byte uniform)
 *   compute pass dispatch             (renderer.ts:421-431)          -> addon.dispatch(ctx, camera, frames)
 *
 * options.devices = [ordinal, ...] puts several GPUs of the node behind the same Renderer (include/ptmi.h ptmi_multi_*): the
 * frame's rows are dealt out as interleaved strips, every device accumulates its own, and the frame is assembled on the first
 * device by one RCCL gather — when it is read (readOutput / blit), and every options.gatherEvery frames for a preview.
 *
 * The frame loop (start) paces itself: the reference's is paced by requestAnimationFrame (renderer.ts:456-473); here a tick
 * first waits until at most one earlier dispatch is unfinished (two in flight with the new one), and while the camera stands
 * still it doubles the frames per dispatch up to options.maxFramesPerTick (64) — ptmi_dispatch(camera, n) IS n single-frame
 * dispatches (include/ptmi.h), so the image is the reference's, at the rate of large batches; any camera change drops to 1.
 *
 * The blit pass, tweakpane stats and the DOM controller are out of scope (SURVEY.md §8).
 * Plain JavaScript (Node >= 12: no optional chaining), typed by index.d.ts.
 */
var path = require('path');
var pack = require('./pack');
var sceneFile = require('./scene_file');

var addon = null;
function loadAddon() {
  if (!addon) addon = require(path.join(__dirname, 'addon', 'ptmi_napi.node'));   // throws if not built
  return addon;
}

var MAX_FRAMES = -1;                       // renderer.ts:16

function Renderer(options) {
  options = options || {};
  this.addon = loadAddon();
  this.api = this.addon;                                // the same functions under the name callers poll, e.g. api.throttle(ctx, n)
  this.multi = !!options.devices;
  // throws without a gfx950 device: there is no CPU path
  this.ctx = this.multi ? this.addon.multiCreate(options.devices, options.loopback ? 1 : 0) : this.addon.create(options.device || 0);
  this.gatherEvery = options.gatherEvery || 0;          // several devices: assemble the frame every so many frames (0: when it is read)
  this.sinceGather = 0;
  this.maxFramesPerTick = options.maxFramesPerTick || 64;
  this.framesPerTick = 1;
  this.width = options.width || 800;
  this.height = options.height || 600;
  this.frameIndex = 0;
  this.onUpdateTasks = [];
  this.timer = null;
  this.lastTime = 0;
  this.sceneLoaded = false;
  this.alphaCutout = !!options.alphaCutout;             // loadModel of a .glb keeps albedo alpha and sets the MASK materials' cutoffs
  this.alphaLayers = options.alphaLayers || 0;          // ... with this maxLayers (0: the library's default)
  this.alphaBlend = !!options.alphaBlend;               // loadModel of a .glb keeps albedo alpha and sets the BLEND materials' factors
  this.alphaBlendSeed = options.alphaBlendSeed || 0;    // ... with this seed, and alphaLayers as their maxLayers
  this.cameraBytes = new ArrayBuffer(pack.CAMERA_SIZE);
  this.setupCamera();
  this.addon.resize(this.ctx, this.width, this.height);
  if (options.options) this.addon.setOptions(this.ctx, options.options);
  this.adaptive = null;
  this.adaptiveActive = -1;                 // pixels the last adaptive round listed (-1: none issued since the last reset)
  this.reproject = null;                    // setReproject: the parameters, while camera changes carry the accumulated samples over
  this.accumulatedUnder = null;             // the camera bytes of the last adaptive round: what the planes were accumulated under
  this.reprojectFrom = null;                // ... kept here while a camera change waits for the next round to reproject
  this.rebuildAbove = options.rebuildAbove || 0;        // updateTriangles rebuilds the walked tree above this costNow / costBuilt (0: never)
  this.motion = false;                      // setMotion: reprojection carries the samples across updateTriangles too
  this.projections = !!options.projections; // the camera's projection words are honoured (setProjection, useSceneCamera)
  if (this.projections) this.addon.setProjections(this.ctx, true);
  if (options.adaptive) this.setAdaptive(options.adaptive);
}

/** renderer.ts:136-150 */
Renderer.prototype.setupCamera = function () {
  this.camera = {
    position: [0, 1.0, 2.8], forward: [0, 0, -1], right: [1, 0, 0], up: [0, 1, 0],
    fov: Math.PI / 3, aspect: this.width / this.height, width: this.width, height: this.height,
    frameIndex: 0, focusDistance: 5.0, aperture: 0.001,
  };
};

/** The camera's projection (include/ptmi.h ptmi_set_projections): 'perspective' (the reference's pinhole: camera.fov),
 *  'orthographic' (params.ymag: the half-height in world units, finite and > 0; the half-width is ymag * aspect) or 'equirect' (the
 *  full sphere about camera.position: longitude across the width, latitude up the height; a 2:1 frame gives square degrees). Needs
 *  new Renderer({projections: true}): without it the library does not read the camera's projection words. forward / right / up must
 *  be orthonormal. 'equirect' cannot be combined with setReproject: its inverse is outside the library's arithmetic contract. Restarts
 *  accumulation. */
Renderer.prototype.setProjection = function (kind, params) {
  if (!(kind in pack.PROJECTIONS)) throw new Error("setProjection: 'perspective', 'orthographic' or 'equirect', not " + kind);
  if (!this.projections && kind !== 'perspective') throw new Error('setProjection needs new Renderer({projections: true})');
  if (kind === 'equirect' && this.reproject) throw new Error('an equirectangular camera cannot be reprojected: call setReproject(null) first');
  var ymag = params && params.ymag !== undefined ? Number(params.ymag) : this.camera.ymag || 0;
  if (kind === 'orthographic' && !(ymag > 0 && isFinite(ymag))) throw new Error('setProjection: orthographic needs a finite ymag > 0');
  this.camera.projection = kind; this.camera.ymag = ymag;
  this.resetOutputBuffer(false);
};

/** The cameras of the loaded .glb (scene_prep.js: name, type, position, forward, right, up, and yfov / aspectRatio / znear or xmag /
 *  ymag). useSceneCamera(i) looks through camera i: position, basis, fov or ymag, and the projection. The frame keeps its size: where
 *  the file's aspect ratio differs from the frame's, the vertical extent (yfov / ymag) is kept and the frame's aspect is used. znear
 *  and zfar are not modelled. An orthographic camera needs new Renderer({projections: true}). */
Renderer.prototype.sceneCameras = function () { return (this.sceneInfo && this.sceneInfo.cameras) || []; };
Renderer.prototype.useSceneCamera = function (i) {
  var cams = this.sceneCameras();
  if (!(i >= 0 && i < cams.length)) throw new Error('useSceneCamera: the scene has ' + cams.length + ' cameras, no camera ' + i);
  var kind = lookThrough(this.camera, cams[i]);
  this.setProjection(kind, { ymag: this.camera.ymag });
};
/** what useSceneCamera sets on a camera object from a scene camera entry: position, basis, and fov (perspective) or ymag
 *  (orthographic). aspect, width and height stay the frame's. Returns the projection's name. */
function lookThrough(cam, c) {
  cam.position = c.position.slice(); cam.forward = c.forward.slice(); cam.right = c.right.slice(); cam.up = c.up.slice();
  if (c.type === 'orthographic') { cam.ymag = c.ymag; cam.projection = 'orthographic'; }
  else { cam.fov = c.yfov; cam.projection = 'perspective'; }
  return cam.projection;
}

Renderer.prototype.addOnUpdate = function (callback) { this.onUpdateTasks.push(callback); };

/**
 * renderer.ts:130-134. `model` is a .glb path (loaded and prepared like loader.ts + gpu.ts do), a
 * .ptscene path, {blobs, atlas} from readSceneFile / prepareScene, or a SceneData object
 * (gpu.ts:60-65) which is packed here like renderer.ts:282-320 does.
 */
Renderer.prototype.loadModel = function (model, atlas) {
  var self = this;
  return new Promise(function (resolve) {
    var blobs, cutoff = null, blend = null, groups = null, skin = null, morph = null;
    self.gltf = null; self.skins = null; self.morphs = null; self.lightmapUvs = null;
    if (typeof model === 'string' && /\.glb$/i.test(model)) {
      var gltf = require('./gltf').loadGLB(model);
      var prepared = require('./scene_prep').prepareScene(gltf, { alphaCutout: self.alphaCutout, alphaBlend: self.alphaBlend });
      blobs = prepared.blobs; atlas = atlas || prepared.atlas; self.sceneInfo = prepared;
      cutoff = prepared.alphaCutoff || null;
      blend = prepared.alphaBlend || null;
      groups = prepared.triangleGroups || null;
      self.lightmapUvs = prepared.lightmapUvs || null;
      if (prepared.skinTriangles) { skin = prepared; self.gltf = gltf; }
      if (prepared.morphTriangles) { morph = prepared; self.gltf = gltf; }
    } else if (typeof model === 'string') {
      var f = sceneFile.readSceneFile(model);
      blobs = f.blobs; atlas = atlas || f.atlas;
    } else if (model.blobs) {
      blobs = model.blobs; atlas = atlas || model.atlas;
      groups = model.triangleGroups || null;                            // what prepareScene returned: a triangle's glTF node
      self.lightmapUvs = model.lightmapUvs || null;                     // ... and its lightmap coordinates
      if (model.skinTriangles) { skin = model; self.gltf = model.gltf || null; }   // ... and its skinned triangles
      if (model.morphTriangles) { morph = model; self.gltf = model.gltf || null; } // ... and its morphed ones
      if (self.alphaCutout) cutoff = model.alphaCutoff || null;         // what prepareScene({alphaCutout: true}) returned
      if (self.alphaBlend) blend = model.alphaBlend || null;            // ... and prepareScene({alphaBlend: true})
    } else {
      blobs = pack.packScene(model);
    }
    self.addon.uploadScene(self.ctx, blobs.triangles, blobs.materials, blobs.bvhNodes, blobs.lights);
    self.sceneTriangles = blobs.triangles;            // bake() rasterises them
    self.sceneBounds = rootBox(blobs.bvhNodes);       // setMedium({ bounds: 'scene' })
    if (atlas) self.addon.uploadAtlas(self.ctx, atlas.data, atlas.width, atlas.height, atlas.format || 1);
    else self.addon.uploadAtlas(self.ctx, null, 0, 0, 0);
    // (the upload removed any table: it belonged to the old scene's materials)
    if (cutoff) self.addon.setAlphaCutoff(self.ctx, cutoff, self.alphaLayers);
    if (blend) self.addon.setAlphaBlend(self.ctx, blend, self.alphaLayers, self.alphaBlendSeed);
    // ... and any group table: a .glb's triangles are tagged with the node they came from (transformGroups moves a node by matrix)
    if (groups && groups.length) self.addon.setTriangleGroups(self.ctx, groups);
    // ... and any skin: a .glb's skinned primitives are listed with their joints and weights (poseSkin / poseAt pose them)
    if (skin && skin.skinTriangles.length) {
      self.addon.setSkin(self.ctx, skin.skinTriangles, skin.skinCorners, skin.skinJoints);
      self.skins = skin;
    }
    // ... and any morph: a .glb's primitives with targets are listed with their deltas (poseMorph / poseAt pose them)
    if (morph && morph.morphTriangles.length) {
      self.addon.setMorph(self.ctx, morph.morphTriangles, morph.morphRowStart, morph.morphDeltas, morph.morphTargets);
      self.morphs = morph;
    }
    self.sceneLoaded = true;
    self.resetOutputBuffer(false);
    resolve();
  });
};

/** the box of the hierarchy's root, node 0 of the 48-byte nodes (min.xyz, pad, max.xyz, pad, ...); null without nodes */
function rootBox(bvhNodes) {
  var bytes = bvhNodes && (bvhNodes.byteLength || 0);
  if (!bytes || bytes < 32) return null;
  var f = bvhNodes instanceof ArrayBuffer ? new Float32Array(bvhNodes, 0, 8)
                                          : new Float32Array(bvhNodes.buffer, bvhNodes.byteOffset, 8);
  return { min: [f[0], f[1], f[2]], max: [f[4], f[5], f[6]] };
}

/** renderer.ts:357-366. cameraMoved: the reset follows a camera change and nothing else; with setReproject and adaptive rounds
 *  accumulated, the samples then stay, for the next round to reproject from the camera they were accumulated under. */
Renderer.prototype.resetOutputBuffer = function (restart, cameraMoved) {
  this.reprojectFrom = cameraMoved && this.reproject && this.adaptive && this.frameIndex > 0 ? this.accumulatedUnder : null;
  if (!this.reprojectFrom) this.frameIndex = 0;
  this.camera.frameIndex = 0;
  this.framesPerTick = 1;                   // the picture changed: back to one frame per tick, for the shortest latency
  this.adaptiveActive = -1;
  this.adaptivePending = false;
  if (restart !== false && this.timer === null && this.sceneLoaded) this.start();
};

/** renderer.ts:403-413 */
Renderer.prototype.updateCamera = function () {
  this.camera.frameIndex = this.frameIndex;
  pack.packCamera(this.camera, this.cameraBytes);
};

/** renderer.ts:415-454 (compute pass only). frames > 1 traces that many consecutive frames in one call. */
Renderer.prototype.renderFrame = function (frames) {
  frames = frames || 1;
  this.updateCamera();
  if (this.motion && this.frameIndex === 0) this.addon.motionCommit(this.ctx);     // a restart: the history is rendered with the current geometry
  this.addon.dispatch(this.ctx, this.cameraBytes, frames);
  this.frameIndex += frames;
  if (this.multi && this.gatherEvery > 0) {
    this.sinceGather += frames;
    if (this.sinceGather >= this.gatherEvery) { this.addon.gather(this.ctx); this.sinceGather = 0; }
  }
};

/** renderer.ts:456-473 — requestAnimationFrame becomes setImmediate */
Renderer.prototype.start = function () {
  var self = this;
  this.lastTime = Date.now();
  var animate = function () {
    // Back-pressure without blocking the event loop (the reference's requestAnimationFrame loop never blocks: input events keep
    // flowing): POLL how many dispatches are unfinished and come back on the next turn of the loop while more than one is — at
    // most two in flight with the one a tick enqueues. A turn that only waits is not a tick: no update task runs.
    if (self.sceneLoaded && self.addon.throttle(self.ctx, 0xFFFFFFFF) > 1) {
      self.throttledTurns = (self.throttledTurns || 0) + 1;
      if (self.timer !== null) self.timer = setImmediate(animate);
      return;
    }
    var now = Date.now();
    var dt = (now - self.lastTime) / 1000;
    self.lastTime = now;
    for (var i = 0; i < self.onUpdateTasks.length; i++) self.onUpdateTasks[i](dt);      // may move the camera: framesPerTick = 1
    if (self.timer === null) return;        // an update task stopped the loop
    if (self.adaptive) {
      // adaptive: one round in flight. Whether anything is left is read once the throttle's poll says that round has finished (the
      // status call then finds the device idle), so a turn of the loop never waits for a round; until then it only re-arms.
      if (self.adaptivePending && self.addon.throttle(self.ctx, 0xFFFFFFFF) === 0) {
        self.adaptiveActive = self.adaptiveStatus().active;
        self.adaptivePending = false;
      }
      if (self.adaptiveActive === 0) { self.timer = null; return; }      // converged: no re-arming until the picture changes
      if (!self.adaptivePending) { self.renderAdaptive(1); self.adaptivePending = true; }
    } else if (MAX_FRAMES === -1 || self.frameIndex < MAX_FRAMES) {
      var n = self.framesPerTick;
      if (MAX_FRAMES !== -1) n = Math.min(n, MAX_FRAMES - self.frameIndex);
      self.renderFrame(n);
      self.framesPerTick = Math.min(self.framesPerTick * 2, self.maxFramesPerTick);     // still camera: larger batches
    }
    if (self.timer !== null) self.timer = setImmediate(animate);
  };
  this.timer = setImmediate(animate);
};

Renderer.prototype.stop = function () {
  if (this.timer !== null) { clearImmediate(this.timer); this.timer = null; }
};

/** renderer.ts:482-494 */
Renderer.prototype.destroy = function () {
  this.stop();
  if (this.ctx) { this.addon.destroy(this.ctx); this.ctx = null; }
};

/** renderer.ts:496-510 */
/**
 * The environment map behind every miss (include/ptmi.h ptmi_upload_environment): float32 RGBA texels, equirectangular, row 0 at the
 * +Y pole. opts: { intensity (0 / undefined: 1), rotation (radians about +Y), sample (0: next-event estimation samples it, 1: lookup
 * only) }. texels null removes it. Accumulation restarts: the picture under another sky is another picture.
 */
Renderer.prototype.setEnvironment = function (texels, width, height, opts) {
  opts = opts || {};
  if (texels && !(texels instanceof Float32Array)) throw new TypeError('setEnvironment: texels must be a Float32Array of RGBA');
  this.addon.uploadEnvironment(this.ctx, texels || null, texels ? width : 0, texels ? height : 0,
                               { intensity: opts.intensity || 0, rotation: opts.rotation || 0, sample: opts.sample ? 1 : 0 });
  this.frameIndex = 0;
};

/**
 * One homogeneous scattering medium inside an axis-aligned box (include/ptmi.h ptmi_set_medium): { sigmaT (extinction per unit
 * length), albedo (a number or [r, g, b], default 1), g (Henyey-Greenstein asymmetry, default 0), bounds ({ min: [x, y, z],
 * max: [x, y, z] }, or 'scene': the root box of the scene loaded last) }. null removes it. Accumulation restarts.
 */
Renderer.prototype.setMedium = function (medium) {
  if (!medium) {
    this.addon.setMedium(this.ctx, null);
    this.mediumSet = null;                  // (the library drops the density grid with its medium)
    this.densityScale = 1;
  } else {
    var bounds = medium.bounds;
    if (bounds === 'scene') {
      if (!this.sceneBounds) throw new Error("setMedium: bounds 'scene' needs a loaded scene with a hierarchy");
      bounds = this.sceneBounds;
    }
    if (!bounds || !bounds.min || !bounds.max) throw new TypeError("setMedium: bounds must be { min, max } or 'scene'");
    var a = medium.albedo === undefined ? 1 : medium.albedo;
    var m = { sigmaT: medium.sigmaT, albedo: typeof a === 'number' ? [a, a, a] : a, g: medium.g || 0, min: bounds.min, max: bounds.max };
    var scale = this.densityScale || 1;     // a normalised density grid in place: its maximum stays in sigma_t
    this.addon.setMedium(this.ctx, scale === 1 ? m : Object.assign({}, m, { sigmaT: m.sigmaT * scale }));
    this.mediumSet = m;
  }
  this.frameIndex = 0;
};

/**
 * Edits of the loaded scene in place (include/ptmi.h ptmi_update_triangles / _materials / _lights): `blob` holds whole records in the
 * layout loadModel uploads (an ArrayBuffer or a typed array), written over the scene's from record `first` on. The topology stays:
 * same counts, same triangle order. updateTriangles refits the trees on the device and refreshes sceneBounds (what
 * setMedium({ bounds: 'scene' }) reads) from the refitted root box; sceneUpdateStatus().costNow / costBuilt says how far the refitted
 * tree has degraded, for the host to decide when to rebuildTree (new Renderer({ rebuildAbove: ratio }) does so here). Accumulation restarts, except after updateTriangles under
 * setReproject, setMotion(true) and adaptive rounds, which continues (setMotion). A refused edit throws and changes nothing.
 */
Renderer.prototype.updateTriangles = function (first, blob) {
  if (!this.sceneLoaded) throw new Error('updateTriangles: needs a loaded scene (loadModel)');
  this.addon.updateTriangles(this.ctx, first, blob);
  this._trianglesEdited();
};
/** what follows every edit of the triangles: the scene bounds, the accumulation, the rebuild above options.rebuildAbove */
Renderer.prototype._trianglesEdited = function () {
  var st = this.addon.sceneUpdateStatus(this.ctx);
  if (this.sceneBounds) this.sceneBounds = { min: st.rootMin, max: st.rootMax };
  if (this.motion && this.reproject && this.adaptive && this.frameIndex > 0 && this.accumulatedUnder) {
    // setReproject and setMotion: the samples stay, and the next round is preceded by a reprojection from the camera they were
    // accumulated under (the current one, unless a camera change is waiting too) that follows the moved triangles
    if (!this.reprojectFrom) this.reprojectFrom = this.accumulatedUnder;
    this.adaptiveActive = -1;
    this.adaptivePending = false;
  } else this.frameIndex = 0;
  if (this.rebuildAbove > 0 && st.costBuilt > 0 && st.costNow / st.costBuilt > this.rebuildAbove) this.rebuildTree();
};
Renderer.prototype.updateMaterials = function (first, blob) {
  if (!this.sceneLoaded) throw new Error('updateMaterials: needs a loaded scene (loadModel)');
  this.addon.updateMaterials(this.ctx, first, blob);
  this.frameIndex = 0;
};
Renderer.prototype.updateLights = function (first, blob) {
  if (!this.sceneLoaded) throw new Error('updateLights: needs a loaded scene (loadModel)');
  this.addon.updateLights(this.ctx, first, blob);
  this.frameIndex = 0;
};
/**
 * Objects moved on the device (include/ptmi.h ptmi_set_triangle_groups / ptmi_transform_groups). setTriangleGroups tags every triangle
 * of the loaded scene with a group id (a Uint32Array in the uploaded order; null removes the table) and snapshots the rest pose;
 * loadModel of a .glb does it with the index of the node each triangle came from (scene.triangleGroups). transformGroups sets
 * matrices: [{ group, matrix (12 numbers: a 3 x 4 row-major affine), normalMatrix? (9 numbers; derived through ptmi_normal_matrix
 * when absent) }]. Transforms are absolute, from the rest pose; 96 bytes per group cross the bus. What follows is what follows
 * updateTriangles: bounds, accumulation (kept under setMotion with setReproject and adaptive rounds), options.rebuildAbove.
 * A refused call throws and changes nothing.
 */
Renderer.prototype.setTriangleGroups = function (groups) {
  if (groups && !(groups instanceof Uint32Array)) throw new TypeError('setTriangleGroups: groups must be a Uint32Array or null');
  if (!this.sceneLoaded) throw new Error('setTriangleGroups: needs a loaded scene (loadModel)');
  this.addon.setTriangleGroups(this.ctx, groups || null);
};
Renderer.prototype.transformGroups = function (ops) {
  if (!this.sceneLoaded) throw new Error('transformGroups: needs a loaded scene (loadModel)');
  var blob = new ArrayBuffer(96 * ops.length), u32 = new Uint32Array(blob), f32 = new Float32Array(blob);
  for (var i = 0; i < ops.length; i++) {
    var op = ops[i], m = Float32Array.from(op.matrix), nm = new Float32Array(9);
    if (m.length !== 12) throw new RangeError('transformGroups: matrix must hold 12 numbers (3 x 4, row-major)');
    if (op.normalMatrix) {
      if (op.normalMatrix.length !== 9) throw new RangeError('transformGroups: normalMatrix must hold 9 numbers');
      nm.set(op.normalMatrix);
    } else this.addon.normalMatrix(this.ctx, m, nm);
    u32[24 * i] = op.group;
    f32.set(m, 24 * i + 2);
    f32.set(nm, 24 * i + 14);
  }
  this.addon.transformGroups(this.ctx, blob);
  this._trianglesEdited();
};
/** { present, nGroups, transforms, lastMoved, firstBad, transformMs } of the group table in place */
Renderer.prototype.transformStatus = function () {
  return this.addon.transformStatus(this.ctx);
};
/**
 * Skinned meshes posed on the device (include/ptmi.h ptmi_set_skin / ptmi_pose_skin). setSkin lists the skinned triangles (a
 * Uint32Array of ascending indices in the uploaded order; null removes the skin) with three 32-byte corner records each (corners: an
 * ArrayBuffer of { uint32 joint[4], float32 weight[4] }) for a skeleton of nJoints, and snapshots the rest pose; loadModel of a .glb
 * with skins does it (scene.skinTriangles / skinCorners). poseSkin takes a complete pose, one entry per joint in joint order:
 * [{ matrix (12 numbers: a 3 x 4 row-major affine), normalMatrix? (9 numbers; derived through ptmi_normal_matrix when absent) }].
 * Poses are absolute, from the rest pose; 96 bytes per joint cross the bus. What follows is what follows updateTriangles.
 * A refused call throws and changes nothing.
 */
Renderer.prototype.setSkin = function (triangles, corners, nJoints) {
  if (triangles && !(triangles instanceof Uint32Array)) throw new TypeError('setSkin: triangles must be a Uint32Array or null');
  if (!this.sceneLoaded) throw new Error('setSkin: needs a loaded scene (loadModel)');
  this.addon.setSkin(this.ctx, triangles || null, triangles ? corners : null, nJoints >>> 0);
  this.skins = null;                                                   // (poseAt poses the skin loadModel set, not this one)
};
Renderer.prototype.poseSkin = function (joints) {
  if (!this.sceneLoaded) throw new Error('poseSkin: needs a loaded scene (loadModel)');
  var blob = new ArrayBuffer(96 * joints.length), u32 = new Uint32Array(blob), f32 = new Float32Array(blob);
  for (var i = 0; i < joints.length; i++) {
    var j = joints[i], m = Float32Array.from(j.matrix), nm = new Float32Array(9);
    if (m.length !== 12) throw new RangeError('poseSkin: matrix must hold 12 numbers (3 x 4, row-major)');
    if (j.normalMatrix) {
      if (j.normalMatrix.length !== 9) throw new RangeError('poseSkin: normalMatrix must hold 9 numbers');
      nm.set(j.normalMatrix);
    } else this.addon.normalMatrix(this.ctx, m, nm);
    u32[24 * i] = i;
    f32.set(m, 24 * i + 2);
    f32.set(nm, 24 * i + 14);
  }
  this.addon.poseSkin(this.ctx, blob);
  this._trianglesEdited();
};
/** { present, nJoints, nSkinned, poses, firstBad, poseMs } of the skin in place */
Renderer.prototype.skinStatus = function () {
  return this.addon.skinStatus(this.ctx);
};
/**
 * Morphed meshes posed on the device (include/ptmi.h ptmi_set_morph / ptmi_pose_morph). setMorph lists the morphed triangles (a
 * Uint32Array of ascending indices in the uploaded order; null removes the morph) with a sparse table of 96-byte delta records in
 * compressed-row form (rowStart: one word more than triangles; deltas: an ArrayBuffer of ptmi_morph_delta records, ascending by target
 * within a row) for nTargets targets, and snapshots the rest pose; loadModel of a .glb with morph targets does it. poseMorph takes one
 * weight per target; poses are absolute, and targets of weight zero cost nothing. Triangles the skin lists too are handed to the
 * skin's rest pose and reach the live records at the next poseSkin (morph, then skin: glTF's order). A refused call throws and changes
 * nothing.
 */
Renderer.prototype.setMorph = function (triangles, rowStart, deltas, nTargets) {
  if (triangles && !(triangles instanceof Uint32Array)) throw new TypeError('setMorph: triangles must be a Uint32Array or null');
  if (triangles && rowStart && !(rowStart instanceof Uint32Array)) throw new TypeError('setMorph: rowStart must be a Uint32Array');
  if (!this.sceneLoaded) throw new Error('setMorph: needs a loaded scene (loadModel)');
  this.addon.setMorph(this.ctx, triangles || null, triangles ? rowStart || null : null, triangles ? deltas || null : null, nTargets >>> 0);
  this.morphs = null;                                                  // (poseAt poses the morph loadModel set, not this one)
};
Renderer.prototype.poseMorph = function (weights) {
  if (!this.sceneLoaded) throw new Error('poseMorph: needs a loaded scene (loadModel)');
  this.addon.poseMorph(this.ctx, Float32Array.from(weights));
  this._trianglesEdited();
};
/** { present, nTargets, nMorphed, nRecords, nInSkin, poses, activeTargets, firstBad, skinStale, poseMs } of the morph in place */
Renderer.prototype.morphStatus = function () {
  return this.addon.morphStatus(this.ctx);
};
/** poses the loaded .glb at t seconds of its animation animationIndex: the animated local transforms and morph weights (animation.js
 *  sample: STEP and LINEAR); the morph first (scene_prep.morphPose, then poseMorph), then the skin: the node hierarchy composed in
 *  double, the joint matrices of scene_prep.skinPose, then poseSkin */
Renderer.prototype.poseAt = function (animationIndex, t) {
  if ((!this.skins && !this.morphs) || !this.gltf) throw new Error('poseAt: needs a loaded .glb with a skin or morph targets (loadModel)');
  var animation = require('./animation'), prep = require('./scene_prep');
  var locals = animation.sample(this.gltf, animationIndex, t);
  if (this.morphs) this.poseMorph(prep.morphPose(this.morphs, locals));
  if (this.skins) this.poseSkin(prep.skinPose(this.skins, animation.worldMatrices(this.gltf, locals)));
};
/** { updates, quantisedKept, planMs, refitMs, costBuilt, costNow, rootMin, rootMax } of the triangle updates since loadModel */
Renderer.prototype.sceneUpdateStatus = function () {
  return this.addon.sceneUpdateStatus(this.ctx);
};

/**
 * The walked tree rebuilt in place (include/ptmi.h ptmi_rebuild_tree): a refit keeps the topology, so the tree degrades as geometry
 * moves; this builds the own-leaf tree anew from the triangles as they stand on the device and swaps it in, leaving the triangle
 * order, the tables, the alpha table, the motion state and every plane alone. opts: { builder (1 the host's, 2 / 0 / absent the
 * device's where it applies) }. Any tree over the same triangles gives the same hits, so the accumulated samples stay valid and
 * frameIndex is kept. Returns rebuildStatus(). new Renderer({ rebuildAbove: ratio }) calls this after an updateTriangles that leaves
 * costNow / costBuilt above the ratio: off by default; a rebuild was measured to pay from roughly 1.2 - 1.3 (README.md). Throws for
 * an image without own leaves (options.leaves = 1, keepReferenceTree).
 */
Renderer.prototype.rebuildTree = function (opts) {
  if (!this.sceneLoaded) throw new Error('rebuildTree: needs a loaded scene (loadModel)');
  this.addon.rebuildTree(this.ctx, (opts && opts.builder) || 0);
  return this.addon.rebuildStatus(this.ctx);
};
/** { rebuilds, builderUsed, buildMs, costBefore, costAfter } of the rebuilds since loadModel */
Renderer.prototype.rebuildStatus = function () {
  return this.addon.rebuildStatus(this.ctx);
};

/**
 * Alpha cutouts (include/ptmi.h ptmi_set_alpha_cutoff): a Float32Array with one cutoff per material of the loaded scene — 0 opaque,
 * > 0: a hit is absent where the albedo map's alpha is below it (glTF alphaMode MASK) — or null to remove the table. opts:
 * { maxLayers (holes one ray may pass per segment, 1 .. 32; 0 / absent: the default, 4) }. new Renderer({ alphaCutout: true }) does
 * this on loadModel of a .glb from its materials' alphaMode / alphaCutoff. loadModel removes the table. Accumulation restarts.
 */
Renderer.prototype.setAlphaCutoff = function (cutoff, opts) {
  if (cutoff && !(cutoff instanceof Float32Array)) throw new TypeError('setAlphaCutoff: cutoff must be a Float32Array or null');
  if (cutoff && !this.sceneLoaded) throw new Error('setAlphaCutoff: needs a loaded scene (loadModel)');
  this.addon.setAlphaCutoff(this.ctx, cutoff || null, (opts && opts.maxLayers) || 0);
  this.frameIndex = 0;
};
/** { present, materials, cutout, maxLayers, pathPasses, pathExhausted, shadowPasses, shadowExhausted } (include/ptmi.h
 *  ptmi_alpha_status): the table in place and what its loops counted since resetStats; synchronises */
Renderer.prototype.alphaStatus = function () { return this.addon.alphaStatus(this.ctx); };

/**
 * Alpha blending as hashed stochastic transparency (include/ptmi.h ptmi_set_alpha_blend): a Float32Array with one entry per material
 * of the loaded scene, < 0 not blended, f in [0, 1]: a hit is absent where f * the albedo map's alpha is at or below a hash of the ray
 * (glTF alphaMode BLEND, f = baseColorFactor[3]), or null to remove the table. opts: { maxLayers (absent hits one ray may pass per
 * segment, 1 .. 32; 0 / absent: the default, 4), seed (the hash's last word; absent: 0) }. new Renderer({ alphaBlend: true }) does this
 * on loadModel of a .glb from its materials. loadModel removes the table. Accumulation restarts.
 */
Renderer.prototype.setAlphaBlend = function (factor, opts) {
  if (factor && !(factor instanceof Float32Array)) throw new TypeError('setAlphaBlend: factor must be a Float32Array or null');
  if (factor && !this.sceneLoaded) throw new Error('setAlphaBlend: needs a loaded scene (loadModel)');
  this.addon.setAlphaBlend(this.ctx, factor || null, (opts && opts.maxLayers) || 0, (opts && opts.seed) || 0);
  this.frameIndex = 0;
};
/** { present, materials, blend, maxLayers, seed, pathTests, pathPasses, shadowTests, shadowPasses } (include/ptmi.h
 *  ptmi_alpha_blend_status): the table in place and what the loops counted for it since resetStats; synchronises */
Renderer.prototype.alphaBlendStatus = function () { return this.addon.alphaBlendStatus(this.ctx); };

/** why ptmi_upload_medium_density would refuse rho over dims on medium m with sigmaT times scale (include/ptmi.h), or null */
function refusal(rho, dims, m, scale) {
  var n = 1;
  for (var k = 0; k < 3; k++) {
    if (!(dims[k] >= 1 && dims[k] <= 1024) || dims[k] !== Math.floor(dims[k])) return 'dimension ' + dims[k] + ' is not an integer in 1 .. 1024';
    n *= dims[k];
  }
  if (rho.length < n) return 'the array holds ' + rho.length + ' values, the grid ' + n;
  for (var i = 0; i < n; i++) if (!(rho[i] >= 0 && rho[i] <= 1)) return 'density ' + rho[i] + ' at entry ' + i + ' is not within [0, 1]';
  var sigma = Math.fround(m.sigmaT * scale), d2 = 0;
  if (!(sigma > 0 && isFinite(sigma))) return 'sigmaT ' + sigma + ' is not finite and > 0';
  for (var a = 0; a < 3; a++) { var e = Math.fround(m.max[a]) - Math.fround(m.min[a]); d2 += e * e; }
  if (!(sigma * Math.sqrt(d2) <= 256)) return 'sigmaT * |box diagonal| = ' + sigma * Math.sqrt(d2) + ' exceeds 256, the limit of a medium with a density grid';
  return null;
}

/**
 * A density grid for the medium in place (include/ptmi.h ptmi_upload_medium_density): a Float32Array of nx * ny * nz multipliers of
 * the medium's sigmaT, x fastest, stretched over its box; dims = [nx, ny, nz]; opts: { filter ('nearest', the default, or 'linear'),
 * normalise (false: the values must lie in [0, 1]; true: any non-negative densities: they are divided by their maximum, and the
 * medium's sigmaT is multiplied by it, so that sigmaT * rho stays what the array says) }. rho null removes the grid, and the medium is
 * homogeneous with the sigmaT it was set with. Needs setMedium first. A refused grid throws and leaves the grid and the medium in place,
 * also where `normalise` would have changed sigmaT. Accumulation restarts.
 */
Renderer.prototype.setMediumDensity = function (rho, dims, opts) {
  opts = opts || {};
  var self = this;
  function rescale(scale) {                 // sigmaT of the medium as it was set, times scale
    if (scale !== (self.densityScale || 1)) {
      self.addon.setMedium(self.ctx, Object.assign({}, self.mediumSet, { sigmaT: self.mediumSet.sigmaT * scale }));
      self.densityScale = scale;
    }
  }
  if (!rho) {
    this.addon.uploadMediumDensity(this.ctx, null, [0, 0, 0], 0);
    if (this.mediumSet) rescale(1);
  } else {
    if (!(rho instanceof Float32Array)) throw new TypeError('setMediumDensity: rho must be a Float32Array');
    if (!dims || dims.length !== 3) throw new TypeError('setMediumDensity: dims must be [nx, ny, nz]');
    if (!this.mediumSet) throw new Error('setMediumDensity: needs a medium in place (setMedium)');
    if (opts.filter !== undefined && opts.filter !== 'nearest' && opts.filter !== 'linear') throw new TypeError("setMediumDensity: filter must be 'nearest' or 'linear'");
    var scale = 1;
    if (opts.normalise) {
      var max = 0;
      for (var i = 0; i < rho.length; i++) {
        if (!(rho[i] >= 0 && isFinite(rho[i]))) throw new RangeError('setMediumDensity: density ' + rho[i] + ' at entry ' + i + ' is not finite and >= 0');
        if (rho[i] > max) max = rho[i];
      }
      if (max > 0) {
        scale = max;
        var scaled = new Float32Array(rho.length);
        for (var j = 0; j < rho.length; j++) scaled[j] = Math.min(rho[j] / max, 1);
        rho = scaled;
      }
    }
    var filter = opts.filter === 'linear' ? 1 : 0;
    if (scale === (this.densityScale || 1)) {
      this.addon.uploadMediumDensity(this.ctx, rho, [dims[0], dims[1], dims[2]], filter);       // a refused grid leaves the one in place
    } else {
      // Another scale: the grid in place was normalised for the old one, so it has to go before sigmaT changes. What the library would
      // refuse is therefore refused here first, before anything changes: like a failed ptmi_upload_medium_density, a throw leaves
      // the grid and the medium in place.
      var why = refusal(rho, dims, this.mediumSet, scale);
      if (why) throw new RangeError('setMediumDensity: ' + why);
      this.addon.uploadMediumDensity(this.ctx, null, [0, 0, 0], 0);
      rescale(scale);
      this.addon.uploadMediumDensity(this.ctx, rho, [dims[0], dims[1], dims[2]], filter);
    }
  }
  this.frameIndex = 0;
};

Renderer.prototype.resize = function (width, height) {
  this.width = width; this.height = height;
  this.camera.aspect = width / height;
  this.camera.width = width; this.camera.height = height;
  this.reprojectFrom = null;                // the planes of the new size are empty
  this.frameIndex = 0;
  this.framesPerTick = 1;
  this.addon.resize(this.ctx, width, height);
};

/** renderer.ts:152-170 */
Renderer.prototype.moveCamera = function (forward, right, up) {
  var c = this.camera;
  for (var k = 0; k < 3; k++) c.position[k] += right * c.right[k] + forward * c.forward[k] + up * c.up[k];
  this.resetOutputBuffer(undefined, true);
};

function normalize(v) { var l = Math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); return [v[0] / l, v[1] / l, v[2] / l]; }
function cross(a, b) { return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]; }

/** renderer.ts:172-201: yaw about +Y, then the clamped pitch delta about +X */
Renderer.prototype.rotateCamera = function (yaw, pitch) {
  var c = this.camera;
  var currentPitch = Math.asin(c.forward[1]);
  var lim = (Math.PI / 2) * 0.99;
  var newPitch = Math.max(Math.min(currentPitch + pitch, lim), -lim);
  var dp = newPitch - currentPitch;
  var f = c.forward;
  var cx = Math.cos(dp), sx = Math.sin(dp);                 // v1 = Rx(dp) v
  var v1 = [f[0], cx * f[1] - sx * f[2], sx * f[1] + cx * f[2]];
  var cy = Math.cos(yaw), sy = Math.sin(yaw);               // v2 = Ry(yaw) v1
  c.forward = normalize([cy * v1[0] + sy * v1[2], v1[1], -sy * v1[0] + cy * v1[2]]);
  c.right = normalize(cross(c.forward, [0, 1, 0]));
  c.up = normalize(cross(c.right, c.forward));
  this.resetOutputBuffer(undefined, true);
};

/** Output buffer (binding 0): width*height float4, row 0 = image bottom. Synchronises. */
Renderer.prototype.readOutput = function () {
  var out = new Float32Array(this.width * this.height * 4);
  this.addon.readOutput(this.ctx, out);
  return out;
};

/**
 * A lightmap of the loaded scene (include/ptmi.h ptmi_upload_bake_surface, ptmi_dispatch_bake, ptmi_bake_dilate): opts = { width,
 * height (default: the frame's), frames (samples per texel, default 64), dilate (gutter-fill passes, default 0), bias (default 1e-6),
 * denoise (true, or { iterations, phiColor, phiNormal, phiPosition }, 0 or absent: the default; include/ptmi.h ptmi_bake_denoise) }.
 * The scene's triangles are rasterised over their lightmap coordinates (bake.js: a .glb's TEXCOORD_1, else TEXCOORD_0; any other
 * model: the triangles' own uv0..2), every covered texel traces `frames` paths from its surface point, and the result is the
 * width * height float4 lightmap, index y * width + x with row y at lightmap coordinate v = (y + 0.5) / height: the mean incoming
 * radiance under the cosine law, E / pi, which the engine multiplies by albedo. w is 0, or with dilate > 0 the texel's state: 1
 * covered, 2 filled, 0 empty. With denoise the result is the filtered lightmap (w: the state, gutter-filled when dilate > 0): the
 * sample-moments plane is on for the length of the bake and as it was afterwards. Texels lie where the triangles were when they were loaded: later edits and poses are traced but do not
 * move them. One device only; the first-hit planes must be off. The frame takes the lightmap's size (resize) and accumulation
 * restarts; lastBake = { width, height, frames, covered } (and denoised: true after a filtered one) says what was baked. Synchronises.
 */
Renderer.prototype.bake = function (opts) {
  opts = opts || {};
  if (!this.sceneLoaded || !this.sceneTriangles) throw new Error('bake: needs a loaded scene (loadModel)');
  if (this.multi) throw new Error('bake: one device only');
  if (this.aovMask) throw new Error('bake: turn the first-hit planes off first (setAovs([]), setDenoise(false), setReproject(null))');
  var W = opts.width || this.width, H = opts.height || this.height;
  var frames = opts.frames === undefined ? 64 : opts.frames;
  var t = this.sceneTriangles;
  var f = t instanceof ArrayBuffer ? new Float32Array(t) : new Float32Array(t.buffer, t.byteOffset, Math.floor(t.byteLength / 4));
  var n = Math.floor(f.length / 32);
  var positions = new Float32Array(9 * n), normals = new Float32Array(9 * n), uvs = this.lightmapUvs;
  var own = !uvs || uvs.length !== 6 * n;
  if (own) uvs = new Float32Array(6 * n);
  for (var i = 0; i < n; i++)
    for (var c = 0; c < 3; c++) {
      for (var k = 0; k < 3; k++) {
        positions[9 * i + 3 * c + k] = f[32 * i + 4 * c + k];
        normals[9 * i + 3 * c + k] = f[32 * i + 12 + 4 * c + k];
      }
      if (own) { uvs[6 * i + 2 * c] = f[32 * i + 24 + 2 * c]; uvs[6 * i + 2 * c + 1] = f[32 * i + 25 + 2 * c]; }
    }
  var surface = require('./bake').rasterise(positions, normals, uvs, W, H);
  this.stop();
  if (W !== this.width || H !== this.height) this.resize(W, H);
  this.addon.uploadBakeSurface(this.ctx, surface.texels, W, H);
  var out = new Float32Array(W * H * 4);
  var denoise = opts.denoise ? (typeof opts.denoise === 'object' ? opts.denoise : {}) : null;
  var momentsWere = this.addon.getMoments(this.ctx);
  try {
    if (denoise && !momentsWere) this.addon.setMoments(this.ctx, true);   // the filter's variance: folded during the bake
    this.addon.writeOutput(this.ctx, out);                              // uncovered texels read as zeros
    this.addon.dispatchBake(this.ctx, { firstFrame: 0, bias: opts.bias === undefined ? 1e-6 : opts.bias }, frames);
    if (denoise)
      this.addon.bakeDenoise(this.ctx, { iterations: denoise.iterations || 0, dilate: opts.dilate > 0 ? opts.dilate : 0,
        phiColor: denoise.phiColor || 0, phiNormal: denoise.phiNormal || 0, phiPosition: denoise.phiPosition || 0 }, out);
    else if (opts.dilate > 0) this.addon.bakeDilate(this.ctx, opts.dilate, out);
    else this.addon.readOutput(this.ctx, out);
  } finally {
    if (denoise && !momentsWere) this.addon.setMoments(this.ctx, false);
    this.addon.uploadBakeSurface(this.ctx, null, 0, 0);
  }
  this.lastBake = { width: W, height: H, frames: frames, covered: surface.covered };
  if (denoise) this.lastBake.denoised = true;
  this.reprojectFrom = null;
  this.frameIndex = 0;                      // the output buffer holds a lightmap now: a camera's accumulation starts over
  return out;
};

/**
 * Light probes of the loaded scene (include/ptmi.h ptmi_upload_probes, ptmi_dispatch_probes, ptmi_probe_sh, ptmi_probe_irradiance):
 * opts = { positions (3 numbers per probe) | grid: { min, max, counts } (probes.js: cell centres), enabled (flags per probe, default
 * all), tile (N, default 8), frames (samples per atlas texel, default 64), irradiance (m, default 0: none) }. Every texel of every
 * enabled probe's N x N tile traces `frames` paths from the probe along its octahedral direction. Returns { radiance: the
 * width * height float4 atlas (probe i owns tile (i % cols, i / cols), row 0 at the bottom), sh: 27 floats per probe (k major, rgb
 * minor), irradiance: m * m float4 per probe (E / pi, w = 1) or null, width, height, count }. One device only; the first-hit planes
 * must be off. The frame takes the atlas's size (probes.js atlasSize) and accumulation restarts. Synchronises.
 * visibility: { tile (m), sharpness (log2 of the lobe's exponent, default 6), maxDistance (default: probes.js maxDistance of the grid),
 * border (default false) } additionally gathers the depth plane (ptmi_set_probe_depth) and returns depth: the width * height float4
 * plane (mean distance, mean squared distance, hit fraction, 0), and visibility: (m + 2 * border)^2 float4 per probe
 * (ptmi_probe_visibility; INTEGRATION.md 1.21 has the shader's test). With border the irradiance tiles get their ring of wrapped
 * texels too (probes.js addBorder): (m + 2)^2 float4 per probe.
 */
Renderer.prototype.bakeProbes = function (opts) {
  opts = opts || {};
  var probes = require('./probes');
  if (!this.sceneLoaded) throw new Error('bakeProbes: needs a loaded scene (loadModel)');
  if (this.multi) throw new Error('bakeProbes: one device only');
  if (this.aovMask) throw new Error('bakeProbes: turn the first-hit planes off first (setAovs([]), setDenoise(false), setReproject(null))');
  var positions = opts.positions || (opts.grid && probes.grid(opts.grid.min, opts.grid.max, opts.grid.counts));
  if (!positions || positions.length < 3) throw new Error('bakeProbes: positions or grid');
  var count = Math.floor(positions.length / 3);
  var tile = opts.tile || 8, frames = opts.frames === undefined ? 64 : opts.frames, m = opts.irradiance || 0;
  var size = probes.atlasSize(count, tile), W = size.width, H = size.height;
  var vis = opts.visibility || null, visMax = 0;
  if (vis) {
    visMax = vis.maxDistance || (opts.grid ? probes.maxDistance(opts.grid.min, opts.grid.max, opts.grid.counts) : 0);
    if (!(visMax > 0)) throw new Error('bakeProbes: visibility.maxDistance (positions have no lattice to take it from)');
    if (!vis.tile) throw new Error('bakeProbes: visibility.tile');
  }
  this.stop();
  if (W !== this.width || H !== this.height) this.resize(W, H);
  this.addon.uploadProbes(this.ctx, probes.records(positions, opts.enabled), tile);
  var radiance = new Float32Array(W * H * 4), sh = new Float32Array(count * 27), irr = m ? new Float32Array(count * m * m * 4) : null;
  var depth = null, visibility = null;
  try {
    if (vis) {
      this.addon.setProbeDepth(this.ctx, visMax);
      depth = new Float32Array(W * H * 4);
      this.addon.writeProbeDepth(this.ctx, depth);                      // a plane left on by the caller: this gather's alone
    }
    this.addon.writeOutput(this.ctx, radiance);                         // tiles of disabled probes read as zeros
    this.addon.dispatchProbes(this.ctx, { firstFrame: 0 }, frames);
    this.addon.readOutput(this.ctx, radiance);
    this.addon.probeSh(this.ctx, sh);
    if (irr) this.addon.probeIrradiance(this.ctx, m, irr);
    if (vis) {
      var side = vis.tile + (vis.border ? 2 : 0);
      this.addon.readProbeDepth(this.ctx, depth);
      visibility = new Float32Array(count * side * side * 4);
      this.addon.probeVisibility(this.ctx, { m: vis.tile, sharpness: vis.sharpness === undefined ? 6 : vis.sharpness, border: vis.border ? 1 : 0 },
                                 visibility);
      if (irr && vis.border) irr = probes.addBorder(irr, m);
    }
  } finally {
    if (vis) this.addon.setProbeDepth(this.ctx, null);
    this.addon.uploadProbes(this.ctx, null, 0);
  }
  this.reprojectFrom = null;
  this.frameIndex = 0;                      // the output buffer holds a probe atlas now: a camera's accumulation starts over
  return { radiance: radiance, sh: sh, irradiance: irr, depth: depth, visibility: visibility, width: W, height: H, count: count };
};

/** The reference's blit pass (renderer.ts:434-449, blit.wgsl): tone-mapped 8-bit canvas, row 0 = top. */
Renderer.prototype.blit = function () {
  var out = new Uint8Array(this.width * this.height * 4);
  this.addon.blit(this.ctx, out);
  return out;
};

/** First-hit planes (include/ptmi.h ptmi_set_aovs): names of the planes to keep from now on, any of 'albedo', 'normal', 'id';
 *  [] turns them all off. With several devices every device keeps its own strips and readAov assembles the plane on the first. */
var AOVS = { albedo: 1, normal: 2, id: 4 };
function aovBit(name) {
  if (!Object.prototype.hasOwnProperty.call(AOVS, name)) throw new Error('unknown AOV plane "' + name + '" (albedo, normal, id)');
  return AOVS[name];
}
Renderer.prototype.setAovs = function (names) {
  var mask = 0;
  (names || []).forEach(function (n) { mask |= aovBit(n); });
  this.addon.setAovs(this.ctx, mask);
  this.aovMask = mask;
};
/** A plane as width*height entries, index y*width+x like readOutput: 'albedo' / 'normal' a Float32Array of 4 per pixel
 *  ((albedo, coverage) / (normal, depth)), 'id' a Uint32Array of 2 (triangle, material; 0xFFFFFFFF on a miss). Synchronises. */
Renderer.prototype.readAov = function (name) {
  var bit = aovBit(name);
  var n = this.width * this.height;
  var out = bit === 4 ? new Uint32Array(n * 2) : new Float32Array(n * 4);
  this.addon.readAov(this.ctx, bit, out);
  return out;
};
/** What is under canvas pixel (x, y), row 0 = top like blit(): {triangle, material, depth} of the last frame traced, or null
 *  on a miss. Needs the 'id' plane; depth (the mean first-hit distance) comes from the 'normal' plane when that is on, else null. */
Renderer.prototype.pick = function (x, y) {
  if (!((this.aovMask || 0) & 4)) throw new Error("pick: turn the 'id' plane on first (setAovs)");
  x = Math.floor(x); y = Math.floor(y);
  if (x < 0 || y < 0 || x >= this.width || y >= this.height) return null;
  var i = (this.height - 1 - y) * this.width + x;           // the planes' row 0 is the image bottom
  var ids = this.readAov('id');
  if (ids[2 * i] === 0xFFFFFFFF) return null;
  var depth = null;
  if (this.aovMask & 2) depth = this.readAov('normal')[4 * i + 3];
  return { triangle: ids[2 * i], material: ids[2 * i + 1], depth: depth };
};

/** The denoiser's inputs (include/ptmi.h ptmi_denoise): on turns the 'normal' and 'albedo' planes and the sample-moments plane on,
 *  off turns the three off; an 'id' plane that is on stays on. Like setAovs, planes turned on mid-accumulation mix with zeros
 *  until the next frame 0. With several devices denoise() first gathers the planes the filter reads onto the first device. */
Renderer.prototype.setDenoise = function (on) {
  var mask = ((this.aovMask || 0) & 4) | (on ? 3 : 0) | (this.reproject ? 2 : 0);      // reprojection keeps the 'normal' plane it reads
  this.addon.setAovs(this.ctx, mask);
  this.aovMask = mask;
  if (on || !this.adaptive) this.addon.setMoments(this.ctx, !!on);      // adaptive sampling keeps the moments plane it counts in
  this.denoiseOn = !!on;
};
/** The denoised output buffer: width*height float4 (rgb, 0), row 0 = image bottom like readOutput. params (all optional, 0 = the
 *  default): {iterations, demodulate, phiColor, phiNormal, phiDepth}. Needs setDenoise(true). Synchronises. */
Renderer.prototype.denoise = function (params) {
  var out = new Float32Array(this.width * this.height * 4);
  this.addon.denoise(this.ctx, params || null, out);
  return out;
};
/** blit() of the last denoise() result: tone-mapped 8-bit canvas, row 0 = top */
Renderer.prototype.blitDenoised = function () {
  var out = new Uint8Array(this.width * this.height * 4);
  this.addon.blitDenoised(this.ctx, out);
  return out;
};

/** Adaptive sampling (include/ptmi.h ptmi_dispatch_adaptive): params = { threshold, floor, minFrames, maxFrames, step,
 *  neighbourhood } (0 or absent: the default; threshold has none), or null to go back to uniform frames. Turns the sample-moments
 *  plane on. While set, the frame loop issues adaptive rounds and stops re-arming once a round lists no pixel. */
Renderer.prototype.setAdaptive = function (params) {
  if (params) {
    if (!(params.threshold > 0)) throw new RangeError('setAdaptive: threshold must be > 0');
    if (!this.denoiseOn && !this.adaptive) this.addon.setMoments(this.ctx, true);
  } else if (this.adaptive && !this.denoiseOn) this.addon.setMoments(this.ctx, false);
  this.adaptive = params || null;
  this.resetOutputBuffer(false);
};
/** `rounds` adaptive rounds; frameIndex counts rounds here (0 restarts, like a first frame) */
Renderer.prototype.renderAdaptive = function (rounds) {
  if (!this.adaptive) throw new Error('renderAdaptive: setAdaptive first');
  rounds = rounds || 1;
  this.updateCamera();
  if (this.motion && this.frameIndex === 0) this.addon.motionCommit(this.ctx);     // a restart: the history is rendered with the current geometry
  if (this.reprojectFrom) {                 // the camera moved since the last round: carry the samples over, then continue
    this.addon.reproject(this.ctx, this.reprojectFrom, this.cameraBytes, this.reproject);
    this.reprojectFrom = null;
  }
  this.addon.dispatchAdaptive(this.ctx, this.cameraBytes, this.adaptive, rounds);
  this.accumulatedUnder = this.reproject ? this.cameraBytes.slice(0) : null;
  this.frameIndex += rounds;
};
/** Reprojection (include/ptmi.h ptmi_reproject): params = { maxHistory, depthTolerance, matchIds } (0 or absent: the default; {} for
 *  all defaults), or null to go back to restarting on every camera change. While set and adaptive sampling is on, moveCamera /
 *  rotateCamera keep the accumulated samples: the next adaptive round is preceded by reproject(previous camera, current camera) and
 *  continues from the per-pixel counts that leaves. Turns the 'normal' plane on (the pass reads its depth); it stays on afterwards. */
Renderer.prototype.setReproject = function (params) {
  if (this.multi) throw new Error('setReproject: reprojection is not supported with several devices');
  if (params && this.camera.projection === 'equirect')
    throw new Error('setReproject: an equirectangular camera cannot be reprojected (setProjection); its inverse is outside the arithmetic contract');
  if (params && !((this.aovMask || 0) & 2)) {
    this.addon.setAovs(this.ctx, (this.aovMask || 0) | 2);
    this.aovMask = (this.aovMask || 0) | 2;
    this.resetOutputBuffer(false);          // a plane turned on mid-accumulation holds zeros until the next frame 0
  }
  this.reproject = params || null;
  if (!params && this.reprojectFrom) this.resetOutputBuffer(false);    // a pending camera change restarts after all
};
/** Motion (include/ptmi.h ptmi_set_motion): while on, the library keeps the vertex positions the history was rendered with, a
 *  reprojection follows the triangles updateTriangles has moved since, and readMotion() returns the per-pixel screen motion. With
 *  setReproject and adaptive sampling on as well, updateTriangles keeps the accumulated samples: the next adaptive round is preceded by
 *  reproject(camera the samples were accumulated under, current camera) and continues from the counts that leaves. The carried
 *  lighting is the old one until new frames dilute it (maxHistory bounds how long). */
Renderer.prototype.setMotion = function (on) {
  if (this.multi) throw new Error('setMotion: reprojection is not supported with several devices');
  this.addon.setMotion(this.ctx, !!on);
  this.motion = !!on;
};
/** The motion plane: width*height float4, row 0 = image bottom like readOutput. Per pixel (x, y): where its surface was under the camera
 *  the last reprojection came from, in pixels relative to the pixel; z: its distance there; w: 0 carried, 1 disoccluded, 2 missed.
 *  Needs setMotion(true). Synchronises. */
Renderer.prototype.readMotion = function () {
  return this.addon.readMotion(this.ctx, new Float32Array(this.width * this.height * 4));
};
/** { on, epochs, dirtyFirst, dirtyCount, moved, movedCarried } (include/ptmi.h ptmi_motion_status); synchronises */
Renderer.prototype.motionStatus = function () { return this.addon.motionStatus(this.ctx); };
/** { carried, disoccluded, missed, samples } of the last reprojection (include/ptmi.h ptmi_reproject_status); synchronises */
Renderer.prototype.reprojectStatus = function () { return this.addon.reprojectStatus(this.ctx); };
/** { active, samples, minCount, maxCount, rounds } (include/ptmi.h ptmi_adaptive_status); synchronises */
Renderer.prototype.adaptiveStatus = function () { return this.addon.adaptiveStatus(this.ctx); };
/** per-pixel sample counts (the moments plane's z): width*height floats, row 0 = image bottom like readOutput */
Renderer.prototype.sampleCounts = function () {
  var m = this.addon.readMoments(this.ctx, new Float32Array(this.width * this.height * 4));
  var out = new Float32Array(this.width * this.height);
  for (var i = 0; i < out.length; i++) out[i] = m[4 * i + 2];
  return out;
};

Renderer.prototype.setOptions = function (o) { this.addon.setOptions(this.ctx, o); };
Renderer.prototype.getStats = function () { return this.addon.getStats(this.ctx); };
/** several devices: assemble the frame on the first one now (readOutput / blit do it themselves) */
Renderer.prototype.gather = function () { this.addon.gather(this.ctx); this.sinceGather = 0; };
Renderer.prototype.synchronize = function () { this.addon.synchronize(this.ctx); };

/** renderer.ts:513-558 without the canvas: create, load, (optionally) start; options.input (an event source,
 *  see controller.js) gets a Controller whose update runs every frame, like renderer.ts:554-555 */
function setupRenderer(options) {
  var r = new Renderer(options);
  if (options && options.input) {
    var controller = new (require('./controller').Controller)(r, options.input);
    r.controller = controller;
    r.addOnUpdate(function (deltaTime) { controller.update(deltaTime); });
  }
  if (!options || !options.model) return Promise.resolve(r);
  return r.loadModel(options.model).then(function () { if (options.autoStart) r.start(); return r; });
}

module.exports = { Renderer: Renderer, setupRenderer: setupRenderer, pack: pack, readSceneFile: sceneFile.readSceneFile,
  atlas: require('./atlas'), decodePNG: require('./png_decode').decodePNG, decodeHDR: require('./hdr_decode').decodeHDR,
  decodeJPEG: require('./jpeg_decode').decodeJPEG, Controller: require('./controller').Controller,
  encodeHDR: require('./hdr_encode').encodeHDR, lookThrough: lookThrough };
