// Types of the Node host. The CPU-side scene types mirror the reference's
// src/renderer/gpu.ts:10-65 and src/renderer/bvh.ts:6-12.
export type Vec2 = ArrayLike<number>;
export type Vec3 = ArrayLike<number>;
export interface AtlasTexture { x: number; y: number; w: number; h: number; }
export interface MaterialCPU {
  baseColor: Vec3; metallic: number; roughness: number; emission: Vec3; emissiveStrength: number;
  ior: number; transmission: number;
  albedoMap: AtlasTexture; normalMap: AtlasTexture; pbrMap: AtlasTexture; emissiveMap: AtlasTexture;
}
export interface TriangleCPU {
  v0: Vec3; v1: Vec3; v2: Vec3; n0: Vec3; n1: Vec3; n2: Vec3; uv0: Vec2; uv1: Vec2; uv2: Vec2; materialIndex: number;
}
export interface CameraCPU {
  position: number[]; forward: number[]; right: number[]; up: number[]; fov: number; aspect: number;
  width: number; height: number; frameIndex: number; aperture: number; focusDistance: number;
  /** the two words the reference pads with (include/ptmi_layout.h): read only by a Renderer made with { projections: true } */
  projection?: Projection | 0 | 1 | 2;
  /** the orthographic half-height in world units (glTF's ymag); the half-width is ymag * aspect */
  ymag?: number;
}
export type Projection = 'perspective' | 'orthographic' | 'equirect';
/** a camera of a loaded .glb, in world space (scene_prep.js sceneCameras): a glTF camera looks down its node's -Z with +Y up */
export interface SceneCamera {
  name: string; node: number; camera: number; type: 'perspective' | 'orthographic';
  position: number[]; forward: number[]; right: number[]; up: number[];
  yfov?: number; aspectRatio?: number; znear?: number; zfar?: number; xmag?: number; ymag?: number;
}
export interface LightCPU { position: Vec3; lightType: number; color: Vec3; intensity: number; triangleIndex: number; }
export interface BVHNode { aabb: { min: Vec3; max: Vec3 }; left: number; right: number; triangleOffset: number; triangleCount: number; }
export interface SceneData { triangles: TriangleCPU[]; materials: MaterialCPU[]; bvhNodes: BVHNode[]; lights: LightCPU[]; }
export interface SceneBlobs { triangles: ArrayBuffer; materials: ArrayBuffer; bvhNodes: ArrayBuffer; lights: ArrayBuffer; }
export interface Atlas { data: ArrayBuffer; width: number; height: number; format: 1 | 2; }
export interface TraceOptions {
  maxBounces?: number; doMis?: number; tileY0?: number; tileY1?: number; framesPerBatch?: number;
  traversal?: 0 | 1 | 2 | 3; cull?: number; timing?: number; keepReferenceTree?: number;
  tileParts?: number; tilePart?: number; tileStrip?: number;
  /** include/ptmi.h: 1 = fast reciprocal / sqrt in `shade` (statistically, not bitwise, the same image); never the default */
  perfMode?: 0 | 1;
  /** 0 / 1 / 2 (library default): run the shadow kernel on a second stream beside the next bounce */
  overlap?: 0 | 1 | 2;
  /** read at loadModel: 0 (library default) / 1 the host builds the traversal hierarchy (SAH) / 2 the GPU does (leaves = 1: linear BVH;
   *  leaves = 2: PLOC over the triangles for scenes above 4 096 triangles, the host below). Same results; stats.treeBuilderUsed
   *  reports who built */
  treeBuilder?: 0 | 1 | 2;
  /** read at loadModel: 0 (library default = 2) / 1 triangles are tested in the uploaded BVH's own leaves / 2 in the library's own
   *  leaves (a SAH hierarchy over the triangles, slivers entered with their reference leaf's box; the winner is verified against its
   *  reference leaf). Results equal mode 1's except, rarely, for rays within ~1e-2 rad of an ordinary triangle's plane (measured:
   *  1 - 4 closest hits per 10^5 such rays aimed at triangle edges; DESIGN.md §3.2 item 4). Mode 1 is the strict mode, and the faster
   *  one on scenes made mostly of thin triangles */
  leaves?: 0 | 1 | 2;
  /** leaves = 2: most triangles per own leaf (0 = library default) */
  leafTris?: number;
}
export interface Stats {
  paths: number; segments: number; shadowRays: number; frames: number; dispatches: number;
  gpuMs: number; extendMs: number; shadeMs: number; shadowMs: number; bvhDepth: number; traversalUsed: number;
  shadowTraced: number; uploadMs: number; framesPerBatchUsed: number; leavesUsed: number; leafTrisUsed: number;
  extendVariant: number; shadowVariant: number; verifyFailed: number;
  /** who built the walked hierarchy at the last loadModel: 1 the host, 2 the GPU, 0 none (the uploaded tree is walked as it is) */
  treeBuilderUsed: number;
}
export class Renderer {
  /** `devices: [0, 1, ...]` renders on several GPUs of one node behind one Renderer (include/ptmi.h ptmi_multi_*: rows dealt out as
   *  interleaved strips, one RCCL gather assembles the frame when it is read, or every `gatherEvery` frames). STATUS: checked with one
   *  device through RCCL and with several contexts on one device (`loopback: true`); more than one device over RCCL has never run —
   *  no machine this was built on has two GPUs. */
  constructor(options?: { device?: number; devices?: number[]; loopback?: boolean; gatherEvery?: number; maxFramesPerTick?: number;
                          width?: number; height?: number; options?: TraceOptions; adaptive?: AdaptiveParams;
                          /** loadModel of a .glb keeps the alpha of albedo maps in the atlas and makes every alphaMode "MASK" material a
                           *  cutout at its alphaCutoff (default 0.5); off (the default): the atlas bytes and everything else as without */
                          alphaCutout?: boolean;
                          /** ... with this maxLayers (0 / absent: the library's default, 4) */
                          alphaLayers?: number;
                          /** loadModel of a .glb keeps the alpha of albedo maps in the atlas and blends every alphaMode "BLEND" material
                           *  with its baseColorFactor[3] as hashed stochastic transparency (setAlphaBlend; maxLayers = alphaLayers);
                           *  off (the default): BLEND materials are opaque */
                          alphaBlend?: boolean;
                          /** ... with this seed (absent: 0) */
                          alphaBlendSeed?: number;
                          /** honour the camera's projection words (include/ptmi.h ptmi_set_projections): what setProjection and an
                           *  orthographic useSceneCamera need. Off by default: every launch and every bit is then as without it */
                          projections?: boolean;
                          /** updateTriangles calls rebuildTree() when it leaves sceneUpdateStatus().costNow / costBuilt above this ratio.
                           *  Off (0 / absent) by default; a rebuild was measured to pay from roughly 1.2 - 1.3 (README.md) */
                          rebuildAbove?: number });
  camera: CameraCPU;
  addOnUpdate(callback: (deltaTime: number) => void): void;
  loadModel(model: string | SceneData | { blobs: SceneBlobs; atlas?: Atlas | null; alphaCutoff?: Float32Array;
                                         alphaBlend?: Float32Array | null }, atlas?: Atlas): Promise<void>;
  /** alpha cutouts (include/ptmi.h ptmi_set_alpha_cutoff): one cutoff per material of the loaded scene, 0 opaque, > 0: a hit is absent
   *  where the albedo map's alpha is below it; null removes the table, and so does loadModel. Restarts accumulation. */
  setAlphaCutoff(cutoff: Float32Array | null, opts?: { maxLayers?: number }): void;
  /** the table in place and what its loops counted since the statistics were reset; synchronises */
  alphaStatus(): AlphaStatus;
  /** alpha blending (include/ptmi.h ptmi_set_alpha_blend): one entry per material of the loaded scene, < 0 not blended, f in [0, 1]: a
   *  hit is absent where f * the albedo map's alpha is at or below a hash of the ray, so it is there with probability alpha and frames
   *  accumulate to the blend; null removes the table, and so does loadModel. Coverage only: no sorting, no coloured transmission.
   *  Restarts accumulation. */
  setAlphaBlend(factor: Float32Array | null, opts?: { maxLayers?: number; seed?: number }): void;
  /** the blend table in place and what the loops counted for it since the statistics were reset; synchronises */
  alphaBlendStatus(): AlphaBlendStatus;
  /** the environment map behind every miss: float32 RGBA texels, equirectangular, row 0 at the +Y pole; null removes it.
   *  Restarts accumulation. */
  setEnvironment(texels: Float32Array | null, width?: number, height?: number, opts?: EnvironmentOptions): void;
  /** one homogeneous scattering medium (fog) inside an axis-aligned box; null removes it. Restarts accumulation. */
  setMedium(medium: MediumOptions | null): void;
  /** a density grid for the medium in place: nx * ny * nz multipliers of its sigmaT, x fastest, stretched over its box; null removes
   *  it. Needs setMedium first. A refused grid throws and leaves the grid and the medium in place. Restarts accumulation. */
  setMediumDensity(rho: Float32Array | null, dims?: [number, number, number], opts?: MediumDensityOptions): void;
  /** writes whole records (the upload's layout) over the loaded scene's from record `first` on and refits the trees on the device;
   *  the topology stays. Refreshes sceneBounds and restarts accumulation. A refused edit throws and changes nothing. */
  updateTriangles(first: number, blob: ArrayBuffer | ArrayBufferView): void;
  updateMaterials(first: number, blob: ArrayBuffer | ArrayBufferView): void;
  updateLights(first: number, blob: ArrayBuffer | ArrayBufferView): void;
  sceneUpdateStatus(): SceneUpdateStatus;
  /** tags every triangle of the loaded scene with a group id, in the uploaded order, and snapshots the rest pose (include/ptmi.h
   *  ptmi_set_triangle_groups); null removes the table. loadModel of a .glb sets the node index of every triangle. */
  setTriangleGroups(groups: Uint32Array | null): void;
  /** sets the matrices of the groups named (ptmi_transform_groups): every member triangle becomes T(rest pose), absolute, and the
   *  trees are refitted on the device. matrix: 12 numbers, a 3 x 4 row-major affine; normalMatrix: 9 numbers, derived through
   *  ptmi_normal_matrix (the cofactors of the upper 3 x 3) when absent. What follows is what follows updateTriangles, rebuildAbove
   *  included. A refused call throws and changes nothing. */
  transformGroups(ops: Array<{ group: number; matrix: ArrayLike<number>; normalMatrix?: ArrayLike<number> }>): void;
  transformStatus(): TransformStatus;
  /** lists the skinned triangles of the loaded scene (ascending indices in the uploaded order) with three 32-byte corner records each
   *  ({ uint32 joint[4], float32 weight[4] }) for a skeleton of nJoints, and snapshots the rest pose (include/ptmi.h ptmi_set_skin);
   *  null removes the skin. loadModel of a .glb with skins does it. */
  setSkin(triangles: Uint32Array | null, corners: ArrayBuffer | ArrayBufferView | null, nJoints: number): void;
  /** a complete pose, one entry per joint in joint order (ptmi_pose_skin): every listed triangle becomes the blend of its joints'
   *  matrices applied to its rest pose, absolute, and the trees are refitted on the device. matrix: 12 numbers, a 3 x 4 row-major
   *  affine; normalMatrix: 9 numbers, derived through ptmi_normal_matrix when absent. A refused call throws and changes nothing. */
  poseSkin(joints: Array<{ matrix: ArrayLike<number>; normalMatrix?: ArrayLike<number> }>): void;
  skinStatus(): SkinStatus;
  /** lists the morphed triangles of the loaded scene (ascending indices in the uploaded order) with their 96-byte delta records in
   *  compressed-row form (rowStart: one word more than triangles; a row ascends by target) for nTargets morph targets, and snapshots
   *  the rest pose (include/ptmi.h ptmi_set_morph); null removes the morph. loadModel of a .glb with morph targets does it. */
  setMorph(triangles: Uint32Array | null, rowStart: Uint32Array | null, deltas: ArrayBuffer | ArrayBufferView | null, nTargets: number): void;
  /** one weight per target (ptmi_pose_morph): every listed triangle becomes its rest pose plus the weighted deltas of its row;
   *  triangles the skin lists too reach the live records at the next poseSkin. Throws, and changes nothing, where a vertex leaves float32. */
  poseMorph(weights: ArrayLike<number>): void;
  morphStatus(): MorphStatus;
  /** poses the loaded .glb at t seconds of its animation: its morph targets first, then its skin (STEP and LINEAR samplers;
   *  CUBICSPLINE throws) */
  poseAt(animationIndex: number, t: number): void;
  /** builds the walked own-leaf tree anew from the triangles as they stand on the device and swaps it in (include/ptmi.h
   *  ptmi_rebuild_tree): the image a fresh loadModel of the edited scene would build, with the triangle order, the tables, the alpha
   *  table, the motion state and every plane left alone. builder: 1 the host's, 2 (default) the device's where it applies. The hits
   *  do not depend on the tree, so accumulation continues. Throws for an image without own leaves (leaves = 1, keepReferenceTree). */
  rebuildTree(opts?: { builder?: 0 | 1 | 2 }): RebuildStatus;
  rebuildStatus(): RebuildStatus;
  /** the root box of the loaded scene's hierarchy (null without one); follows updateTriangles */
  sceneBounds: { min: number[]; max: number[] } | null;
  renderFrame(frames?: number): void;
  start(): void;
  stop(): void;
  destroy(): void;
  resize(width: number, height: number): void;
  moveCamera(forward: number, right: number, up: number): void;
  rotateCamera(yaw: number, pitch: number): void;
  readOutput(): Float32Array;
  /** a lightmap of the loaded scene (include/ptmi.h ptmi_dispatch_bake, ptmi_bake_dilate): its triangles rasterised over their lightmap
   *  coordinates (a .glb's TEXCOORD_1, else TEXCOORD_0; any other model: the triangles' own uv), `frames` paths from every covered
   *  texel. width*height float4, row y at v = (y + 0.5) / height: the mean incoming radiance under the cosine law (E / pi; multiply by
   *  albedo); w is 0, or with dilate > 0 the texel's state (1 covered, 2 filled, 0 empty). Defaults: the frame's size, 64 frames, no
   *  dilation, bias 1e-6. The frame takes the lightmap's size and accumulation restarts. Punctual lights reach a texel only through
   *  later bounces. denoise: true, or the parameters (0 or absent: the default), returns the lightmap filtered over the bake surface
   *  (include/ptmi.h ptmi_bake_denoise), w the texel's state, gutter-filled after the filter when dilate > 0; the sample-moments plane
   *  is on for the bake and as it was afterwards. Throws with several devices and while first-hit planes are on; synchronises */
  bake(opts?: { width?: number; height?: number; frames?: number; dilate?: number; bias?: number;
                denoise?: boolean | { iterations?: number; phiColor?: number; phiNormal?: number; phiPosition?: number } }): Float32Array;
  /** what the last bake() baked; denoised: true after a filtered one */
  lastBake?: { width: number; height: number; frames: number; covered: number; denoised?: boolean };
  /** light probes of the loaded scene (include/ptmi.h ptmi_dispatch_probes, ptmi_probe_sh, ptmi_probe_irradiance): probes at
   *  `positions` (3 numbers each) or at the cell centres of `grid`, each with a tile x tile octahedral tile (default 8) of the atlas
   *  (probe i owns tile (i % cols, i / cols); probes.js atlasSize gives the size), `frames` paths per atlas texel (default 64).
   *  radiance: width*height float4; sh: 27 floats per probe (k major, rgb minor); irradiance: m*m float4 per probe (E / pi, w = 1), or
   *  null without `irradiance: m`. The frame takes the atlas's size and accumulation restarts. Punctual lights reach a probe only
   *  through later bounces. Throws with several devices and while first-hit planes are on; synchronises.
   *  visibility (include/ptmi.h ptmi_set_probe_depth, ptmi_probe_visibility): also depth, width*height float4 (mean distance, mean
   *  squared distance, hit fraction, 0), and visibility, (tile + 2 * border)^2 float4 per probe; sharpness is the log2 of the lobe's
   *  exponent (default 6), maxDistance defaults to 1.5 cell diagonals of `grid`; with border the irradiance tiles get their ring of
   *  wrapped texels too, (m + 2)^2 float4 per probe */
  bakeProbes(opts: { positions?: ArrayLike<number>; grid?: { min: number[]; max: number[]; counts: number[] }; enabled?: ArrayLike<number | boolean>;
                     tile?: number; frames?: number; irradiance?: number;
                     visibility?: { tile: number; sharpness?: number; maxDistance?: number; border?: boolean } | null }):
    { radiance: Float32Array; sh: Float32Array; irradiance: Float32Array | null; depth: Float32Array | null; visibility: Float32Array | null;
      width: number; height: number; count: number };
  /** first-hit planes (include/ptmi.h ptmi_set_aovs); with several devices each keeps its strips and readAov assembles the plane */
  setAovs(names: Array<'albedo' | 'normal' | 'id'>): void;
  /** width*height entries, index y*width+x: 'albedo' / 'normal' 4 floats each, 'id' 2 uint32 (triangle, material) */
  readAov(name: 'albedo' | 'normal'): Float32Array;
  readAov(name: 'id'): Uint32Array;
  /** canvas pixel (row 0 = top): what the last frame hit there, or null on a miss; needs the 'id' plane */
  pick(x: number, y: number): { triangle: number; material: number; depth: number | null } | null;
  /** blit pass (blit.wgsl): tone-mapped RGBA8 canvas, row 0 = top */
  blit(): Uint8Array;
  /** the denoiser's planes (normal, albedo, sample moments) on or off together; an 'id' plane stays; with several devices
   *  denoise() gathers the planes onto the first device and filters the whole frame there */
  setDenoise(on: boolean): void;
  /** adaptive sampling on (params) or off (null): the frame loop then issues adaptive rounds and stops re-arming when a round lists
   *  no pixel; turns the sample-moments plane on. With several devices the rounds select as one device would (include/ptmi.h
   *  ptmi_multi_dispatch_adaptive) */
  setAdaptive(params: AdaptiveParams | null): void;
  /** `rounds` adaptive rounds now (frameIndex 0 restarts) */
  renderAdaptive(rounds?: number): void;
  adaptiveStatus(): { active: number; samples: number; minCount: number; maxCount: number; rounds: number };
  /** reprojection on (params, {} for the defaults) or off (null): while on and adaptive sampling is set, a camera change no longer
   *  restarts the accumulation: the next adaptive round is preceded by reproject(previous camera, current camera) and continues
   *  from the per-pixel counts that leaves (include/ptmi.h ptmi_reproject). Turns the 'normal' plane on; throws with several devices */
  setReproject(params: ReprojectParams | null): void;
  /** 'perspective' (camera.fov), 'orthographic' (params.ymag: the half-height in world units, finite and > 0) or 'equirect' (the full
   *  sphere about camera.position; best with a 2:1 frame). Needs { projections: true }; camera.forward / right / up must be orthonormal.
   *  Throws for 'equirect' while setReproject is set (and setReproject throws under an 'equirect' camera): that inverse is not
   *  implemented. Restarts the accumulation. */
  setProjection(kind: Projection, params?: { ymag?: number }): void;
  /** the cameras of the loaded .glb ([] for any other model) */
  sceneCameras(): SceneCamera[];
  /** looks through camera i of the loaded .glb: position, basis, yfov or ymag, and the projection. The frame keeps its size: where the
   *  file's aspect ratio differs from the frame's, the vertical extent (yfov / ymag) is kept and the frame's aspect is used. znear and
   *  zfar are not modelled. */
  useSceneCamera(i: number): void;
  /** of the last reprojection (include/ptmi.h ptmi_reproject_status); synchronises */
  reprojectStatus(): { carried: number; disoccluded: number; missed: number; samples: number };
  /** motion on / off (include/ptmi.h ptmi_set_motion): while on, a reprojection follows the triangles updateTriangles moved, and with
   *  setReproject and adaptive sampling set as well updateTriangles no longer restarts the accumulation: the next adaptive round is
   *  preceded by a reprojection and continues from the per-pixel counts that leaves. Throws with several devices */
  setMotion(on: boolean): void;
  /** the motion plane, width*height float4, row 0 = image bottom: (x, y) where the pixel's surface was under the camera the last
   *  reprojection came from, in pixels relative to the pixel; z its distance there; w 0 carried / 1 disoccluded / 2 missed.
   *  Needs setMotion(true); synchronises */
  readMotion(): Float32Array;
  /** include/ptmi.h ptmi_motion_status; synchronises */
  motionStatus(): { on: number; epochs: number; dirtyFirst: number; dirtyCount: number; moved: number; movedCarried: number };
  /** per-pixel sample counts (the moments plane's z), width*height, row 0 = image bottom */
  sampleCounts(): Float32Array;
  /** the denoised output buffer (include/ptmi.h ptmi_denoise): width*height float4 (rgb, 0), row 0 = image bottom */
  denoise(params?: DenoiseParams): Float32Array;
  /** blit pass of the last denoise() result: tone-mapped RGBA8 canvas, row 0 = top */
  blitDenoised(): Uint8Array;
  setOptions(o: TraceOptions): void;
  getStats(): Stats;
}
/** 0 or absent: the default (include/ptmi.h ptmi_adaptive_params); threshold is required and > 0 */
export interface AdaptiveParams {
  threshold: number; floor?: number; minFrames?: number; maxFrames?: number; step?: number; neighbourhood?: 0 | 1;
}
/** 0 or absent: the default (include/ptmi.h ptmi_reproject_params) */
export interface ReprojectParams { maxHistory?: number; depthTolerance?: number; matchIds?: 0 | 1 | 2 }
/** 0 or absent: the default (include/ptmi.h ptmi_denoise_params) */
export interface DenoiseParams {
  iterations?: number; demodulate?: 0 | 1 | 2; phiColor?: number; phiNormal?: number; phiDepth?: number;
}
export function setupRenderer(options?: { device?: number; width?: number; height?: number; model?: string; autoStart?: boolean; options?: TraceOptions; input?: InputSource }): Promise<Renderer>;
export const pack: {
  packTriangles(t: TriangleCPU[]): ArrayBuffer; packMaterials(m: MaterialCPU[]): ArrayBuffer;
  packBVH(n: BVHNode[]): ArrayBuffer; packLights(l: LightCPU[]): ArrayBuffer;
  packCamera(c: CameraCPU, out?: ArrayBuffer): ArrayBuffer; packScene(s: SceneData): SceneBlobs;
};
export interface MediumOptions {
  /** extinction per unit length; finite, > 0 */
  sigmaT: number;
  /** single-scattering albedo, a number or [r, g, b], each in [0, 1]; default 1 */
  albedo?: number | [number, number, number];
  /** Henyey-Greenstein asymmetry, |g| <= 0.99; default 0 */
  g?: number;
  /** the medium's box, or 'scene': the root box of the scene loaded last */
  bounds: { min: [number, number, number]; max: [number, number, number] } | 'scene';
}
/** ptmi_alpha_status: passes = holes passed, exhausted = rays still on a hole after maxLayers */
export interface AlphaStatus {
  present: number; materials: number; cutout: number; maxLayers: number;
  pathPasses: number; pathExhausted: number; shadowPasses: number; shadowExhausted: number;
}
/** ptmi_alpha_blend_status: tests = hits on blended materials examined, passes = those found absent */
export interface AlphaBlendStatus {
  present: number; materials: number; blend: number; maxLayers: number; seed: number;
  pathTests: number; pathPasses: number; shadowTests: number; shadowPasses: number;
}
/** ptmi_transform_status: the group table in place and the transforms since it was set */
export interface TransformStatus {
  present: number; nGroups: number; transforms: number; lastMoved: number;
  /** the last call's check pass: the smallest offending triangle, 0xFFFFFFFF for none */
  firstBad: number; transformMs: number;
}
/** ptmi_morph_status: the morph in place and the poses since it was set */
export interface MorphStatus {
  present: number; nTargets: number; nMorphed: number; nRecords: number; nInSkin: number; poses: number; activeTargets: number;
  firstBad: number; skinStale: number; poseMs: number;
}
/** ptmi_skin_status: the skin in place and the poses since it was set */
export interface SkinStatus {
  present: number; nJoints: number; nSkinned: number; poses: number;
  /** the last call's check pass: the smallest offending triangle, 0xFFFFFFFF for none */
  firstBad: number; poseMs: number;
}
/** ptmi_scene_update_status: the triangle updates since the scene was loaded */
export interface SceneUpdateStatus {
  updates: number; quantisedKept: number; planMs: number; refitMs: number;
  /** sum of the walked tree's child-box areas over the root box's area: when the plan was made, and now */
  costBuilt: number; costNow: number;
  /** the refitted root box of the tree as uploaded */
  rootMin: number[]; rootMax: number[];
}
/** ptmi_rebuild_status: the rebuilds of the walked tree since the scene was loaded */
export interface RebuildStatus {
  rebuilds: number;
  /** 1 the host, 2 the device built the last one (0: none yet) */
  builderUsed: number;
  buildMs: number;
  /** the walked tree's cost (SceneUpdateStatus) around the last rebuild */
  costBefore: number; costAfter: number;
}
export interface MediumDensityOptions {
  /** 'nearest' (default): the cell that holds the point; 'linear': trilinear over the cell centres */
  filter?: 'nearest' | 'linear';
  /** false (default): the values must lie in [0, 1]. true: any non-negative densities; they are divided by their maximum and the
   *  medium's sigmaT is multiplied by it */
  normalise?: boolean;
}
export interface EnvironmentOptions {
  /** radiance scale; 0 / undefined: 1 */
  intensity?: number;
  /** radians about +Y, added to the azimuth */
  rotation?: number;
  /** 0 (default): next-event estimation samples the map; 1: misses look it up, nothing samples it */
  sample?: 0 | 1;
}
/** hdr_decode.js — a Radiance .hdr (RGBE) file as float32 RGBA texels, row 0 on top; throws on a malformed or truncated file */
export function decodeHDR(bytes: Uint8Array | ArrayBuffer): { width: number; height: number; data: Float32Array };
export function readSceneFile(path: string): { blobs: SceneBlobs; atlas: Atlas | null };
/** atlas.js — src/renderer/atlas.ts (PackedAtlas): the canvas as RGBA8 and as rgba16float texels, rects per material */
export interface PackedAtlas {
  texture: { width: number; height: number; rgba8: Uint8Array; data: Uint16Array; format: 1 };
  materials: Map<object, { albedoMap: AtlasTexture; normalMap: AtlasTexture; pbrMap: AtlasTexture; emissiveMap: AtlasTexture }>;
}
export const atlas: {
  potpack(boxes: { w: number; h: number; x?: number; y?: number }[]): { w: number; h: number; fill: number };
  /** keepAlpha: albedo maps keep their resampled alpha in the canvas's alpha channel (no other byte differs) */
  packing(gltf: { materials: object[] }, opts?: { keepAlpha?: boolean }): PackedAtlas;
};
export function decodePNG(data: Uint8Array): { width: number; height: number; data: Uint8Array };
/** jpeg_decode.js — sequential and progressive Huffman JPEG, bit-identical to libjpeg-turbo's default decode */
export function decodeJPEG(data: Uint8Array): { width: number; height: number; data: Uint8Array };
/** controller.js — src/renderer/controller.ts without the DOM; events keep the DOM names and payload fields */
export interface InputSource { on(name: string, handler: (event: any) => void): void; off?(name: string, handler: (event: any) => void): void; }
export class Controller {
  constructor(renderer: { moveCamera(f: number, r: number, u: number): void; rotateCamera(yaw: number, pitch: number): void }, source?: InputSource);
  handle(name: 'keydown' | 'keyup' | 'mousemove' | 'touchstart' | 'touchmove' | 'touchend' | 'touchcancel', event: any): void;
  update(deltaTime: number): void;
  destroy(): void;
}
