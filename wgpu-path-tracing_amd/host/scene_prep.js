'use strict';
/**
 * scene_prep.js — glTF -> SceneData, following src/renderer/gpu.ts:67-421 step by step:
 * world matrices by walking up the parent chain (:77-103), per node normal matrix, punctual lights
 * and mesh primitives in node order (:194-299), one material per primitive (:285-291, :356-421),
 * then the SAH-BVH (which sorts the triangles, bvh.ts) and one emissive light per emissive triangle
 * in post-sort order (:121-138). The BVH build and the light list run in libptmi_scene.so through
 * the addon; the result is the four WGSL-layout blobs plus the SceneData-style counts.
 */
var path = require('path');
var M = require('./mat');
var pack = require('./pack');

function addon() { return require(path.join(__dirname, 'addon', 'ptmi_napi.node')); }

/** gpu.ts:153-191 */
function extractNodeMatrix(node) {
  var matrix = node.matrix ? M.create16(node.matrix) : M.identity();
  if (!node.matrix) {
    if (node.translation) M.translate(matrix, M.vec3(node.translation[0], node.translation[1], node.translation[2]), matrix);
    if (node.rotation) {
      var q = new Float32Array(4);
      q[0] = node.rotation[0]; q[1] = node.rotation[1]; q[2] = node.rotation[2]; q[3] = node.rotation[3];
      M.mul(matrix, M.fromQuat(q), matrix);
    }
    if (node.scale) M.scale(matrix, M.vec3(node.scale[0], node.scale[1], node.scale[2]), matrix);
  }
  return matrix;
}

var ZERO_RECT = { x: 0, y: 0, w: 0, h: 0 };

/** gpu.ts:356-421; atlas = Map(material -> {albedoMap, normalMap, pbrMap, emissiveMap}) from atlas.js packing() */
function buildMaterial(material, atlas) {
  if (!material) {
    return {
      baseColor: [1, 1, 1], emission: [0, 0, 0], emissiveStrength: 0.0, metallic: 0.0, roughness: 0.1, ior: 1.5,
      transmission: 0.0, albedoMap: ZERO_RECT, normalMap: ZERO_RECT, pbrMap: ZERO_RECT, emissiveMap: ZERO_RECT,
    };
  }
  var pbr = material.pbrMetallicRoughness || {};
  var ext = material.extensions || {};
  var def = function (v, d) { return v === undefined || v === null ? d : v; };
  var baseColor = def(pbr.baseColorFactor, [1, 1, 1, 1]);
  var emissive = def(material.emissiveFactor, [0, 0, 0]);
  var rects = (atlas && atlas.get(material)) || {};
  return {
    baseColor: [baseColor[0], baseColor[1], baseColor[2]],
    metallic: def(pbr.metallicFactor, 1.0), roughness: def(pbr.roughnessFactor, 1.0),
    emission: [emissive[0], emissive[1], emissive[2]],
    emissiveStrength: def((ext.KHR_materials_emissive_strength || {}).emissiveStrength, 1.0),
    ior: def((ext.KHR_materials_ior || {}).ior, 1.5),
    transmission: def((ext.KHR_materials_transmission || {}).transmissionFactor, 0.0),
    albedoMap: rects.albedoMap || ZERO_RECT, normalMap: rects.normalMap || ZERO_RECT,
    pbrMap: rects.pbrMap || ZERO_RECT, emissiveMap: rects.emissiveMap || ZERO_RECT,
  };
}

/** gpu.ts:301-354 (indexed meshes; a non-indexed mesh throws there too) */
function buildTriangles(position, normal, uv, index) {
  if (!index) throw new Error('No index found');
  uv = uv || new Float32Array(position.length);
  var tris = [];
  for (var i = 0; i < index.length; i += 3) {
    var i0 = index[i] * 3, i1 = index[i + 1] * 3, i2 = index[i + 2] * 3;
    var u0 = index[i] * 2, u1 = index[i + 1] * 2, u2 = index[i + 2] * 2;
    tris.push({
      v0: [position[i0], position[i0 + 1], position[i0 + 2]], v1: [position[i1], position[i1 + 1], position[i1 + 2]],
      v2: [position[i2], position[i2 + 1], position[i2 + 2]],
      n0: [normal[i0], normal[i0 + 1], normal[i0 + 2]], n1: [normal[i1], normal[i1 + 1], normal[i1 + 2]],
      n2: [normal[i2], normal[i2 + 1], normal[i2 + 2]],
      uv0: [uv[u0], uv[u0 + 1]], uv1: [uv[u1], uv[u1 + 1]], uv2: [uv[u2], uv[u2 + 1]], materialIndex: 0,
    });
  }
  return tris;
}

/** gpu.ts:194-299 */
function processNode(gltf, node, allTriangles, allMaterials, allLights, world, atlas, nodeIndex, skinInstance, morphInstance) {
  var normalMat = M.transpose(M.inverse(world));
  if (node.light !== undefined) {
    var light = gltf.lights[node.light];
    var color = light.color ? [light.color[0], light.color[1], light.color[2]] : [1, 1, 1];
    var intensity = light.intensity === undefined || light.intensity === null ? 1.0 : light.intensity;
    if (light.type === 'directional') {
      var rot = M.quatFromMat(world);
      allLights.push({ position: M.transformQuat(M.vec3(0, 0, -1), rot), lightType: 1, color: color, intensity: intensity, triangleIndex: 0 });
    } else if (light.type === 'point') {
      allLights.push({ position: M.transformMat4(M.vec3(0, 0, 0), world), lightType: 2, color: color, intensity: intensity, triangleIndex: 0 });
    }
  }
  if (node.mesh) {
    node.mesh.primitives.forEach(function (prim) {
      var position = prim.attributes.POSITION.value, normal = prim.attributes.NORMAL.value;
      var uv = prim.attributes.TEXCOORD_0 ? prim.attributes.TEXCOORD_0.value : undefined;
      // the lightmap coordinates a bake rasterises (Renderer.bake): glTF's second set, or the first where a file has only one
      var uvLight = prim.attributes.TEXCOORD_1 ? prim.attributes.TEXCOORD_1.value : uv;
      var tp = new Float32Array(position.length), tn = new Float32Array(normal.length);
      for (var i = 0; i < position.length; i += 3) {
        var p = M.transformMat4(M.vec3(position[i], position[i + 1], position[i + 2]), world);
        tp[i] = p[0]; tp[i + 1] = p[1]; tp[i + 2] = p[2];
        var n = M.normalize(M.transformMat4Upper3x3(M.vec3(normal[i], normal[i + 1], normal[i + 2]), normalMat));
        tn[i] = n[0]; tn[i + 1] = n[1]; tn[i + 2] = n[2];
      }
      var tris = buildTriangles(tp, tn, uv, prim.indices ? prim.indices.value : undefined);
      allMaterials.push(buildMaterial(prim.material, atlas));
      // a skinned primitive is still placed by its node's world matrix (the uploaded bytes are what they are without skinning);
      // its triangles remember their three vertices' JOINTS_0 / WEIGHTS_0 for the skin list
      var skinned = skinInstance && prim.attributes.JOINTS_0 && prim.attributes.WEIGHTS_0 && prim.indices;
      // ... and a primitive with morph targets its vertices and the targets' deltas, for the morph list
      var morphed = morphInstance && prim.targets && prim.targets.length && prim.indices;
      tris.forEach(function (t, k) {
        t.materialIndex = allMaterials.length - 1; t.group = nodeIndex;
        if (uvLight && prim.indices) {
          var lx = prim.indices.value, l0 = lx[3 * k] * 2, l1 = lx[3 * k + 1] * 2, l2 = lx[3 * k + 2] * 2;
          t.lightmapUv = [uvLight[l0], uvLight[l0 + 1], uvLight[l1], uvLight[l1 + 1], uvLight[l2], uvLight[l2 + 1]];
        }
        if (skinned) {
          var ix = prim.indices.value;
          t.skin = { instance: skinInstance, vertices: [ix[3 * k], ix[3 * k + 1], ix[3 * k + 2]],
            joints: prim.attributes.JOINTS_0.value, weights: prim.attributes.WEIGHTS_0.value };
        }
        if (morphed) {
          var jx = prim.indices.value;
          t.morph = { instance: morphInstance, vertices: [jx[3 * k], jx[3 * k + 1], jx[3 * k + 2]], targets: prim.targets,
            normal: normal, world: world, normalMat: normalMat };
        }
        allTriangles.push(t);
      });
    });
  }
}

/** glTF's alpha rule for one material as a cutoff of the alpha table (include/ptmi.h ptmi_set_alpha_cutoff): alphaMode "MASK" cuts
 *  at alphaCutoff (default 0.5); "OPAQUE", "BLEND" (opaque under this table: alphaBlendOf) and a primitive without a material are 0 */
function alphaCutoffOf(material) {
  if (!material || material.alphaMode !== 'MASK') return 0;
  return material.alphaCutoff === undefined || material.alphaCutoff === null ? 0.5 : material.alphaCutoff;
}

/** Tags every packed triangle with its group in the padding word at byte 124 (_p6), for the BVH build to carry along: the builder
 *  moves whole 128-byte records (csrc/scene/scene_prep.cpp: std::swap and assignment of ptmi_triangle values, one memcpy of whole
 *  records per split), so the word arrives with its triangle. */
function tagGroups(triangles, allTriangles) {
  var u = new Uint32Array(triangles);
  for (var i = 0; i < allTriangles.length; i++) u[i * 32 + 31] = allTriangles[i].group >>> 0;
}
/** ... and reads the tags back in the reordered order, zeroing the words again: the blob is then the bytes it is without tags */
function untagGroups(triangles) {
  var u = new Uint32Array(triangles), groups = new Uint32Array(u.length / 32);
  for (var i = 0; i < groups.length; i++) { groups[i] = u[i * 32 + 31]; u[i * 32 + 31] = 0; }
  return groups;
}

/** The same ride for the skin: every triangle's PRE-SORT index in a second padding word (byte 92, _p5, behind n2), read back and
 *  zeroed after the build. Only written when the file has a skinned or morphed primitive, or lightmap coordinates to carry. */
var PRESORT_WORD = 23;
function tagPresort(triangles) {
  var u = new Uint32Array(triangles);
  for (var i = 0; i * 32 < u.length; i++) u[i * 32 + PRESORT_WORD] = i;
}
function untagPresort(triangles) {
  var u = new Uint32Array(triangles), at = new Uint32Array(u.length / 32);
  for (var i = 0; i < at.length; i++) { at[i] = u[i * 32 + PRESORT_WORD]; u[i * 32 + PRESORT_WORD] = 0; }
  return at;
}

/** The lightmap coordinates of a prepared scene (Renderer.bake): per triangle in the uploaded (reordered) order, its three corners'
 *  TEXCOORD_1 (TEXCOORD_0 where the primitive has no second set; zeros where it has neither), 6 floats each. */
function lightmapList(allTriangles, presort) {
  var out = new Float32Array(presort.length * 6);
  for (var i = 0; i < presort.length; i++) {
    var uv = allTriangles[presort[i]].lightmapUv;
    if (uv) out.set(uv, 6 * i);
  }
  return out;
}

/** The skin list of a prepared scene (Renderer.setSkin): the uploaded indices of the skinned triangles, ascending, and three 32-byte
 *  corner records each: the vertex's four JOINTS_0 offset by its skin instance's jointBase, and its WEIGHTS_0 normalised to sum 1 in
 *  double and then rounded to float32 (a vertex whose weights sum to 0 keeps them). */
function skinList(allTriangles, presort) {
  var listed = [];
  for (var i = 0; i < presort.length; i++) if (allTriangles[presort[i]].skin) listed.push(i);
  var corners = new ArrayBuffer(96 * listed.length), u32 = new Uint32Array(corners), f32 = new Float32Array(corners);
  listed.forEach(function (at, e) {
    var s = allTriangles[presort[at]].skin;
    for (var c = 0; c < 3; c++) {
      var v = s.vertices[c], sum = 0, k;
      for (k = 0; k < 4; k++) sum += s.weights[4 * v + k];
      for (k = 0; k < 4; k++) {
        u32[24 * e + 8 * c + k] = s.joints[4 * v + k] + s.instance.jointBase;
        f32[24 * e + 8 * c + 4 + k] = sum > 0 ? s.weights[4 * v + k] / sum : s.weights[4 * v + k];
      }
    }
  });
  return { triangles: Uint32Array.from(listed), corners: corners };
}

/** The morph list of a prepared scene (Renderer.setMorph): the uploaded indices of the morphed triangles, ascending, the row bounds and
 *  the 96-byte delta records (include/ptmi.h ptmi_morph_delta), ascending by target within a row, the target offset by its mesh
 *  instance's targetBase. The deltas are brought to the uploaded space: a position delta through the upper 3 x 3 of the node's world
 *  matrix N; a corner's normal delta is the normal matrix applied to dn, divided by the length of that matrix applied to the corner's
 *  local normal (the uploaded normal is that vector normalised), which keeps rest + sum w * delta parallel to the transformed
 *  n + sum w * dn. A target without NORMAL has zero normal deltas; a record whose 18 numbers are all zero is dropped. */
function morphList(allTriangles, presort) {
  var listed = [], rows = [0], recs = [];
  for (var i = 0; i < presort.length; i++) if (allTriangles[presort[i]].morph) listed.push(i);
  listed.forEach(function (at) {
    var m = allTriangles[presort[at]].morph;
    m.targets.forEach(function (target, k) {
      var rec = new Float32Array(24), any = false;
      for (var c = 0; c < 3; c++) {
        var v = 3 * m.vertices[c], d;
        if (target.POSITION) {
          var dp = target.POSITION.value;
          d = M.transformMat4Upper3x3(M.vec3(dp[v], dp[v + 1], dp[v + 2]), m.world);
          rec[4 * c] = d[0]; rec[4 * c + 1] = d[1]; rec[4 * c + 2] = d[2];
        }
        if (target.NORMAL) {
          var dn = target.NORMAL.value;
          var q = M.transformMat4Upper3x3(M.vec3(m.normal[v], m.normal[v + 1], m.normal[v + 2]), m.normalMat);
          var len = Math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
          d = M.transformMat4Upper3x3(M.vec3(dn[v], dn[v + 1], dn[v + 2]), m.normalMat);
          if (len > 0) { rec[12 + 4 * c] = d[0] / len; rec[12 + 4 * c + 1] = d[1] / len; rec[12 + 4 * c + 2] = d[2] / len; }
        }
      }
      for (var w = 0; w < 24; w++) if (rec[w] !== 0) any = true;
      if (!any) return;
      new Uint32Array(rec.buffer)[3] = m.instance.targetBase + k;
      recs.push(rec);
    });
    rows.push(recs.length);
  });
  var deltas = new ArrayBuffer(96 * recs.length), f32 = new Float32Array(deltas);
  recs.forEach(function (r, e) { f32.set(r, 24 * e); });
  return { triangles: Uint32Array.from(listed), rowStart: Uint32Array.from(rows), deltas: deltas };
}

/** The weights of a pose (Renderer.poseMorph) from per-node weights (animation.js sample: out[node].weights): one float per target
 *  of all morphed mesh instances together, a node without weights in `nodes` taking its defaults */
function morphPose(prepared, nodes) {
  var out = new Float32Array(prepared.morphTargets);
  prepared.morphs.forEach(function (m) {
    var w = (nodes && nodes[m.node] && nodes[m.node].weights) || m.weights;
    for (var k = 0; k < m.nTargets; k++) out[m.targetBase + k] = w[k] === undefined ? 0 : w[k];
  });
  return out;
}

/** The joint records of a pose (Renderer.poseSkin) from the world matrix of every node (animation.js worldMatrices: 16 numbers
 *  each, column-major). The rest pose on the device is in world space, placed by the mesh node's world matrix, and glTF poses a
 *  skinned vertex by its joints alone, so the device matrix of joint j is jointWorld_j . inverseBind_j . meshWorld^-1: composed in
 *  double here, rounded to float32 where the records are packed. -> [{ matrix: 12 numbers, 3 x 4 row-major }] by device joint index */
function skinPose(prepared, nodeWorldMatrices) {
  var anim = require('./animation'), out = new Array(prepared.skinJoints);
  prepared.skins.forEach(function (s) {
    s.joints.forEach(function (node, k) {
      var m = nodeWorldMatrices[node];
      if (s.inverseBind) m = anim.mul4(m, Array.prototype.slice.call(s.inverseBind, 16 * k, 16 * k + 16));
      m = anim.mul4(m, s.meshWorldInverse);
      out[s.jointBase + k] = { matrix: [m[0], m[4], m[8], m[12], m[1], m[5], m[9], m[13], m[2], m[6], m[10], m[14]] };
    });
  });
  return out;
}

/** glTF's alpha rule for one material as an entry of the blend table (include/ptmi.h ptmi_set_alpha_blend): alphaMode "BLEND" is
 *  blended with factor baseColorFactor[3] (default 1); every other mode and a primitive without a material are -1, not blended */
function alphaBlendOf(material) {
  if (!material || material.alphaMode !== 'BLEND') return -1;
  var f = (material.pbrMetallicRoughness || {}).baseColorFactor;
  return f && f[3] !== undefined && f[3] !== null ? f[3] : 1;
}

/** The cameras of a file, one entry per node that carries one, in node order: { name, node, camera (the index in gltf.cameras), type,
 *  position, forward, right, up } in world space from the node's world matrix - a glTF camera looks down its node's -Z with +Y up, so
 *  forward / right / up are the normalised images of (0, 0, -1), (1, 0, 0), (0, 1, 0) (orthonormal for a node without scale or shear,
 *  which is what glTF asks of camera nodes) - plus yfov, aspectRatio (undefined: the viewport's), znear for a perspective camera and
 *  xmag, ymag for an orthographic one. znear / zfar are carried for the caller; the renderer clips nothing. */
function sceneCameras(gltf, world) {
  var out = [];
  gltf.nodes.forEach(function (node, nodeIndex) {
    if (!node.camera) return;
    var w = world.get(node), c = node.camera;
    var axis = function (x, y, z) { return Array.from(M.normalize(M.transformMat4Upper3x3(M.vec3(x, y, z), w))); };
    var e = { name: c.name || node.name || 'camera' + out.length, node: nodeIndex, camera: node.cameraIndex, type: c.type,
      position: [w[12], w[13], w[14]], forward: axis(0, 0, -1), right: axis(1, 0, 0), up: axis(0, 1, 0) };
    if (c.type === 'perspective') { e.yfov = c.perspective.yfov; e.aspectRatio = c.perspective.aspectRatio; e.znear = c.perspective.znear; }
    else { e.xmag = c.orthographic.xmag; e.ymag = c.orthographic.ymag; e.znear = c.orthographic.znear; e.zfar = c.orthographic.zfar; }
    out.push(e);
  });
  return out;
}

/** loader.ts:20-40 + gpu.ts:67-150 -> { blobs, atlas, counts, bvhDepth, triangleGroups, groupNames }: triangleGroups holds, per
 *  triangle in the uploaded (reordered) order, the index of the glTF node it came from (Renderer.setTriangleGroups), groupNames
 *  the nodes' names by that index (opts.triangleGroups === false: neither). opts.alphaCutout: the atlas keeps the alpha of albedo maps
 *  and the result carries alphaCutoff, a Float32Array with one cutoff per packed material (else: neither, and every byte as without).
 *  opts.alphaBlend: the atlas keeps that alpha too, and the result carries alphaBlend, a Float32Array with one blend entry per packed
 *  material (alphaBlendOf), or null when no material is BLEND; alphaCutout alone leaves BLEND materials opaque.
 *  A file with skinned primitives (a node with `skin`, JOINTS_0 and WEIGHTS_0) also returns skinTriangles, skinCorners (skinList),
 *  skinJoints (the joints of all skin instances together) and skins: per skinned node { node, skin, joints (node indices),
 *  inverseBind, meshWorldInverse, jointBase } (opts.skins === false, or a file without skins: none of them, and every blob the
 *  same bytes). A file with morph targets also returns morphTriangles, morphRowStart, morphDeltas (morphList), morphTargets (the
 *  targets of all mesh instances together) and morphs: per morphed node { node, targetBase, nTargets, weights (its defaults) }
 *  (opts.morphs === false, or a file without targets: none of them). lightmapUvs: per uploaded triangle its corners' lightmap
 *  coordinates (lightmapList; a file without texture coordinates: undefined). cameras: the file's cameras (sceneCameras; [] without any). */
function prepareScene(gltf, opts) {
  var alphaCutout = !!(opts && opts.alphaCutout), alphaBlend = !!(opts && opts.alphaBlend);
  var packed = require('./atlas').packing(gltf, { keepAlpha: alphaCutout || alphaBlend });
  var allTriangles = [], allMaterials = [], allLights = [], allCutoffs = [], allBlends = [];
  var parent = new Map();
  gltf.nodes.forEach(function (n) { (n.children || []).forEach(function (c) { parent.set(c, n); }); });
  var world = new Map();
  gltf.nodes.forEach(function (node) {
    var w = M.clone(extractNodeMatrix(node));
    var cur = node;
    while (parent.has(cur)) { cur = parent.get(cur); M.mul(extractNodeMatrix(cur), w, w); }
    world.set(node, w);
  });
  var skins = [], skinJoints = 0;
  if (!(opts && opts.skins === false)) gltf.nodes.forEach(function (node, nodeIndex) {
    var skin = node.skin !== undefined && node.mesh ? (gltf.skins || [])[node.skin] : undefined;
    if (!skin) return;
    skins[nodeIndex] = { node: nodeIndex, skin: node.skin, joints: skin.joints, inverseBind: skin.inverseBindMatrices,
      meshWorldInverse: require('./animation').invert4(Array.from(world.get(node))), jointBase: skinJoints };
    skinJoints += skin.joints.length;
  });
  var morphs = [], morphTargets = 0;
  if (!(opts && opts.morphs === false)) gltf.nodes.forEach(function (node, nodeIndex) {
    var anim = require('./animation'), n = anim.targetCount(node);
    if (!n) return;
    morphs[nodeIndex] = { node: nodeIndex, targetBase: morphTargets, nTargets: n, weights: anim.defaultWeights(node) };
    morphTargets += n;
  });
  gltf.nodes.forEach(function (node, nodeIndex) {
    processNode(gltf, node, allTriangles, allMaterials, allLights, world.get(node), packed.materials, nodeIndex, skins[nodeIndex],
      morphs[nodeIndex]);
    // one material per primitive, in the order processNode packs them
    if (alphaCutout && node.mesh) node.mesh.primitives.forEach(function (prim) { allCutoffs.push(alphaCutoffOf(prim.material)); });
    if (alphaBlend && node.mesh) node.mesh.primitives.forEach(function (prim) { allBlends.push(alphaBlendOf(prim.material)); });
  });

  var triangles = pack.packTriangles(allTriangles);             // sorted in place by the BVH build
  var materials = pack.packMaterials(allMaterials);
  var a = addon();
  var grouped = !(opts && opts.triangleGroups === false);       // false: no tags at all, and no table in the result
  if (grouped) tagGroups(triangles, allTriangles);
  var skinned = allTriangles.some(function (t) { return !!t.skin; });
  var morphed = allTriangles.some(function (t) { return !!t.morph; });
  var lightmapped = allTriangles.some(function (t) { return !!t.lightmapUv; });
  if (skinned || morphed || lightmapped) tagPresort(triangles);
  var bvh = a.buildBvh(triangles);
  var triangleGroups = grouped ? untagGroups(triangles) : undefined;
  var presort = skinned || morphed || lightmapped ? untagPresort(triangles) : undefined;
  var skin = skinned ? skinList(allTriangles, presort) : undefined;
  var morph = morphed ? morphList(allTriangles, presort) : undefined;
  var lights = a.emissiveLights(triangles, materials, pack.packLights(allLights));
  return {
    blobs: { triangles: triangles, materials: materials, bvhNodes: bvh.nodes, lights: lights },
    alphaCutoff: alphaCutout ? new Float32Array(allCutoffs) : undefined,
    alphaBlend: alphaBlend ? (allBlends.some(function (f) { return f >= 0; }) ? new Float32Array(allBlends) : null) : undefined,
    triangleGroups: triangleGroups,
    groupNames: grouped ? gltf.nodes.map(function (n, i) { return n.name || 'node' + i; }) : undefined,
    skinTriangles: skin ? skin.triangles : undefined, skinCorners: skin ? skin.corners : undefined,
    skinJoints: skin ? skinJoints : undefined, skins: skin ? skins.filter(Boolean) : undefined,
    morphTriangles: morph ? morph.triangles : undefined, morphRowStart: morph ? morph.rowStart : undefined,
    morphDeltas: morph ? morph.deltas : undefined, morphTargets: morph ? morphTargets : undefined,
    morphs: morph ? morphs.filter(Boolean) : undefined,
    lightmapUvs: lightmapped ? lightmapList(allTriangles, presort) : undefined,
    atlas: packed.texture,
    cameras: sceneCameras(gltf, world),
    counts: { triangles: allTriangles.length, materials: allMaterials.length, bvhNodes: bvh.nodes.byteLength / pack.BVH_NODE_SIZE,
      lights: lights.byteLength / pack.LIGHT_SIZE, punctualLights: allLights.length },
    bvhDepth: bvh.depth,
  };
}

module.exports = { prepareScene: prepareScene, sceneCameras: sceneCameras, skinPose: skinPose, morphPose: morphPose, extractNodeMatrix: extractNodeMatrix, buildMaterial: buildMaterial, alphaCutoffOf: alphaCutoffOf,
  alphaBlendOf: alphaBlendOf };
