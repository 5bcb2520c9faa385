'use strict';
/**
 * animation.js — glTF animations sampled on the host, for skinned meshes posed on the device (Renderer.poseAt; include/ptmi.h
 * ptmi_pose_skin). sample() evaluates the channels of one animation at a time t into per-node local TRS; worldMatrices() composes the
 * node hierarchy. Everything is arithmetic in JS doubles on plain arrays, 4 x 4 matrices column-major as glTF writes them; the one
 * rounding to float32 happens where the joint records are packed (Renderer.poseSkin).
 * Samplers: STEP and LINEAR (rotations by spherical interpolation along the shorter arc). CUBICSPLINE throws. Channels that
 * target morph-target weights are sampled like the others, one number per target per key (Renderer.poseAt; ptmi_pose_morph).
 */

function lerp(a, b, u) { return a.map(function (x, i) { return x + (b[i] - x) * u; }); }

/** unit quaternions (x, y, z, w): the shorter arc, normalised; nearly parallel ones are interpolated linearly */
function slerp(a, b, u) {
  var d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
  if (d < 0) { b = b.map(function (x) { return -x; }); d = -d; }
  var q;
  if (d > 0.9995) q = lerp(a, b, u);
  else {
    var theta = Math.acos(d), s = Math.sin(theta), wa = Math.sin((1 - u) * theta) / s, wb = Math.sin(u * theta) / s;
    q = a.map(function (x, i) { return wa * x + wb * b[i]; });
  }
  var len = Math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  return q.map(function (x) { return x / len; });
}

/** one sampler at t: `width` numbers per key; before the first key its value, after the last the last */
function sampleTrack(sampler, width, t, rotation) {
  if (sampler.interpolation === 'CUBICSPLINE') throw new Error('animation: CUBICSPLINE interpolation is not supported (STEP and LINEAR are)');
  if (sampler.interpolation !== 'STEP' && sampler.interpolation !== 'LINEAR') throw new Error('animation: unknown interpolation ' + sampler.interpolation);
  var times = sampler.input, n = times.length;
  var key = function (k) { return Array.prototype.slice.call(sampler.output, k * width, (k + 1) * width); };
  if (n === 0) throw new Error('animation: a sampler without keys');
  if (t <= times[0]) return key(0);
  if (t >= times[n - 1]) return key(n - 1);
  var k = 0;
  while (times[k + 1] <= t) k++;
  if (sampler.interpolation === 'STEP') return key(k);
  var u = (t - times[k]) / (times[k + 1] - times[k]);
  return rotation ? slerp(key(k), key(k + 1), u) : lerp(key(k), key(k + 1), u);
}

/** how many morph targets the mesh of a node has (0: none) */
function targetCount(node) {
  var n = 0;
  if (node.mesh) node.mesh.primitives.forEach(function (p) { if (p.targets) n = Math.max(n, p.targets.length); });
  return n;
}
/** the morph weights a node has without an animation: its own `weights`, else its mesh's, else zeros; undefined without targets */
function defaultWeights(node) {
  var n = targetCount(node), w = [];
  if (!n) return undefined;
  var given = node.weights || node.mesh.weights || [];
  for (var k = 0; k < n; k++) w.push(given[k] === undefined ? 0 : given[k]);
  return w;
}

/** -> per node { translation, rotation, scale, matrix }: the node's own local transform with the animation's channels at t seconds
 *  laid over it. matrix is the node's `matrix` (16 numbers) where it has one and no channel targets it, else null. A node whose mesh
 *  has morph targets also has `weights`: its default weights (defaultWeights) with a `weights` channel laid over them. */
function sample(gltf, animationIndex, t) {
  var anim = (gltf.animations || [])[animationIndex];
  if (!anim) throw new RangeError('animation: the file has no animation ' + animationIndex);
  var out = gltf.nodes.map(function (n) {
    return { translation: n.translation ? Array.from(n.translation) : [0, 0, 0], rotation: n.rotation ? Array.from(n.rotation) : [0, 0, 0, 1],
      scale: n.scale ? Array.from(n.scale) : [1, 1, 1], matrix: n.matrix ? Array.from(n.matrix) : null };
  });
  gltf.nodes.forEach(function (n, i) { var w = defaultWeights(n); if (w) out[i].weights = w; });
  anim.channels.forEach(function (c) {
    if (c.node === undefined) return;
    if (c.path === 'weights') {
      var width = targetCount(gltf.nodes[c.node]);
      if (width) out[c.node].weights = sampleTrack(anim.samplers[c.sampler], width, t, false);
      return;
    }
    if (c.path !== 'translation' && c.path !== 'rotation' && c.path !== 'scale') throw new Error('animation: unknown path ' + c.path);
    var o = out[c.node];
    o[c.path] = sampleTrack(anim.samplers[c.sampler], c.path === 'rotation' ? 4 : 3, t, c.path === 'rotation');
    o.matrix = null;
  });
  return out;
}

/** a * b (apply b first), column-major */
function mul4(a, b) {
  var d = new Array(16);
  for (var c = 0; c < 4; c++)
    for (var r = 0; r < 4; r++)
      d[c * 4 + r] = a[r] * b[c * 4] + a[4 + r] * b[c * 4 + 1] + a[8 + r] * b[c * 4 + 2] + a[12 + r] * b[c * 4 + 3];
  return d;
}

/** the inverse by Gauss-Jordan elimination with partial pivoting; throws on a singular matrix */
function invert4(m) {
  var a = [], i, j, k;
  for (i = 0; i < 4; i++) { a.push([]); for (j = 0; j < 4; j++) a[i].push(m[j * 4 + i]); for (j = 0; j < 4; j++) a[i].push(i === j ? 1 : 0); }
  for (i = 0; i < 4; i++) {
    var p = i;
    for (k = i + 1; k < 4; k++) if (Math.abs(a[k][i]) > Math.abs(a[p][i])) p = k;
    if (a[p][i] === 0) throw new Error('animation: a singular matrix has no inverse');
    var row = a[p]; a[p] = a[i]; a[i] = row;
    var d = a[i][i];
    for (j = 0; j < 8; j++) a[i][j] /= d;
    for (k = 0; k < 4; k++) {
      if (k === i) continue;
      var f = a[k][i];
      if (f !== 0) for (j = 0; j < 8; j++) a[k][j] -= f * a[i][j];
    }
  }
  var out = new Array(16);
  for (i = 0; i < 4; i++) for (j = 0; j < 4; j++) out[j * 4 + i] = a[i][4 + j];
  return out;
}

/** T * R * S of a sampled node, or its matrix */
function localMatrix(o) {
  if (o.matrix) return o.matrix.slice();
  var x = o.rotation[0], y = o.rotation[1], z = o.rotation[2], w = o.rotation[3], s = o.scale, t = o.translation;
  var xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  return [(1 - 2 * (yy + zz)) * s[0], 2 * (xy + wz) * s[0], 2 * (xz - wy) * s[0], 0,
    2 * (xy - wz) * s[1], (1 - 2 * (xx + zz)) * s[1], 2 * (yz + wx) * s[1], 0,
    2 * (xz + wy) * s[2], 2 * (yz - wx) * s[2], (1 - 2 * (xx + yy)) * s[2], 0,
    t[0], t[1], t[2], 1];
}

/** the world matrix of every node (16 numbers each) from the local transforms sample() returned: parent * local down the hierarchy */
function worldMatrices(gltf, locals) {
  var parent = new Array(gltf.nodes.length).fill(-1), world = new Array(gltf.nodes.length).fill(null);
  gltf.json.nodes.forEach(function (n, i) { (n.children || []).forEach(function (c) { parent[c] = i; }); });
  var of = function (i) {
    if (!world[i]) world[i] = parent[i] < 0 ? localMatrix(locals[i]) : mul4(of(parent[i]), localMatrix(locals[i]));
    return world[i];
  };
  for (var i = 0; i < world.length; i++) of(i);
  return world;
}

/** the file's own pose: every node's local transform as written */
function restPose(gltf) {
  return gltf.nodes.map(function (n) {
    return { translation: n.translation ? Array.from(n.translation) : [0, 0, 0], rotation: n.rotation ? Array.from(n.rotation) : [0, 0, 0, 1],
      scale: n.scale ? Array.from(n.scale) : [1, 1, 1], matrix: n.matrix ? Array.from(n.matrix) : null };
  });
}

module.exports = { defaultWeights: defaultWeights, targetCount: targetCount, sample: sample, worldMatrices: worldMatrices, restPose: restPose, mul4: mul4, invert4: invert4, slerp: slerp };
