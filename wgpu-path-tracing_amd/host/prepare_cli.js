#!/usr/bin/env node
'use strict';
/** prepare_cli.js <model.glb> <outDir>: runs the host's glTF -> SceneData path (gltf.js + atlas.js + scene_prep.js,
 *  i.e. loader.ts + atlas.ts + gpu.ts + bvh.ts of the reference) and writes triangles/materials/bvhNodes/lights
 *  .bin blobs, the atlas (atlas.bin = rgba16float texels, atlas_rgba8.bin = the 8-bit canvas), triangle_groups.bin (one uint32 per
 *  triangle: the glTF node it came from), for a file with skins skin_triangles.bin (the uploaded indices of the skinned triangles,
 *  uint32) and skin_corners.bin (three 32-byte corner records each), for a file with morph targets morph_triangles.bin,
 *  morph_rows.bin (uint32 each) and morph_deltas.bin (96-byte delta records), and info.json (counts, names, and the file's cameras).
 *  No GPU needed. */
var fs = require('fs'), path = require('path');
var s = require('./scene_prep').prepareScene(require('./gltf').loadGLB(process.argv[2]));
var dir = process.argv[3];
Object.keys(s.blobs).forEach(function (k) { fs.writeFileSync(path.join(dir, k + '.bin'), Buffer.from(s.blobs[k])); });
var a = s.atlas;
fs.writeFileSync(path.join(dir, 'atlas.bin'), Buffer.from(a.data.buffer, a.data.byteOffset, a.data.byteLength));
fs.writeFileSync(path.join(dir, 'atlas_rgba8.bin'), Buffer.from(a.rgba8.buffer, a.rgba8.byteOffset, a.rgba8.byteLength));
fs.writeFileSync(path.join(dir, 'triangle_groups.bin'), Buffer.from(s.triangleGroups.buffer));
if (s.skinTriangles) {
  fs.writeFileSync(path.join(dir, 'skin_triangles.bin'), Buffer.from(s.skinTriangles.buffer));
  fs.writeFileSync(path.join(dir, 'skin_corners.bin'), Buffer.from(s.skinCorners));
}
if (s.morphTriangles) {
  fs.writeFileSync(path.join(dir, 'morph_triangles.bin'), Buffer.from(s.morphTriangles.buffer));
  fs.writeFileSync(path.join(dir, 'morph_rows.bin'), Buffer.from(s.morphRowStart.buffer));
  fs.writeFileSync(path.join(dir, 'morph_deltas.bin'), Buffer.from(s.morphDeltas));
}
var skins = s.skins && s.skins.map(function (k) { return { node: k.node, skin: k.skin, joints: k.joints, jointBase: k.jointBase }; });
fs.writeFileSync(path.join(dir, 'info.json'), JSON.stringify({ counts: s.counts, bvhDepth: s.bvhDepth, groupNames: s.groupNames,
  skinJoints: s.skinJoints, skins: skins, morphTargets: s.morphTargets, morphs: s.morphs, cameras: s.cameras,
  atlas: { width: a.width, height: a.height, format: a.format } }));
console.log(JSON.stringify(s.counts));
