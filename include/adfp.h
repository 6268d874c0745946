/*
 * adfp.h -- C ABI of libadfp.so: the MI355X (gfx950) implementation of the per-ray
 * volume-rendering hot path of MachinePerceptionLab/Attentive_DFPrior.
 *
 * The reference offers no C ABI, plugin or operator registry for this path; its boundary
 * is two Python objects (src/DF_Prior.py:50-51 `shared_decoders`, :111 `renderer`).  The
 * entry points below are what a ctypes binding under those two objects calls; each cites the
 * reference function it replaces.  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer owned by the caller (PyTorch) unless it says "host".
 *    The library never allocates, frees or retains device memory.
 *  - All work is enqueued asynchronously on `stream` (a hipStream_t passed as void*).
 *  - Return value: 0 = ok; <0 = argument error detected on the host (ADFP_E_*);
 *    >0 = hipError_t of a failed launch.  No exception crosses the ABI.
 *  - Feature grids are consumed channels-last ([Z][Y][X][32] fp32; one voxel = one 128-B
 *    line); adfp_relayout_grid converts from the reference's [1,32,Z,Y,X] layout
 *    (src/DF_Prior.py:243-264).  The TSDF is consumed in place through element strides, so the
 *    permuted view of get_tsdf.py:95-97 needs no copy.
 *  - Decoder weights are consumed as "packed images" (MFMA operand order)
 *    produced by adfp_pack_decoder / adfp_pack_attention from a flat fp32 buffer that is the
 *    concatenation of the module's parameters in state_dict order (decoder.py:110-166,
 *    :212-228).
 */
#ifndef ADFP_H
#define ADFP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADFP_VERSION 134

/* error codes (host-detected) */
#define ADFP_E_ARG        (-1)   /* null pointer / negative size */
#define ADFP_E_UNSUPPORTED (-2)  /* N_importance>0, occupancy=False, S too large ... */
#define ADFP_E_WORKSPACE  (-3)   /* workspace too small */

/* stage enum: DF.forward(stage=...) decoder.py:307 */
#define ADFP_STAGE_LOW   0
#define ADFP_STAGE_HIGH  1
#define ADFP_STAGE_COLOR 2

/* decoder kinds for packing */
#define ADFP_DEC_LOW   0   /* MLP(name='low',  c_dim=32, color=False) decoder.py:276 */
#define ADFP_DEC_HIGH  1   /* MLP(name='high', c_dim=64, concat_feature) decoder.py:279 */
#define ADFP_DEC_COLOR 2   /* MLP(name='color',c_dim=32, color=True) decoder.py:282 */

/* point source modes for adfp_eval_points */
#define ADFP_PTS_RAYS 0    /* p = rays_o[r] + rays_d[r] * z_vals[r][s]  (Renderer.py:223) */
#define ADFP_PTS_F64  1    /* explicit [P,3] float64 */
#define ADFP_PTS_F32  2    /* explicit [P,3] float32 */

#define ADFP_MAX_SAMPLES 256

typedef struct adfp_grid {
    const float* data;      /* channels-last [Z][Y][X][32] */
    int Z, Y, X;
} adfp_grid;

typedef struct adfp_tsdf {
    const float* data;      /* element (z,y,x) at data[z*sZ + y*sY + x*sX] */
    int Z, Y, X;
    long long sZ, sY, sX;   /* element strides (the reference's view has sZ=1) */
    /* Optional: the CORNER-BLOCK copy of the same volume (adfp_relayout_tsdf), or NULL.  When given, the TSDF stage of the render
     * path (a10 inside adfp_render_forward / adfp_eval_points / adfp_tsdf_stage) reads it instead of `data`: one aligned 32-byte
     * piece per sample wherever the sample lies -- for batches whose neighbouring rays are NOT neighbouring pixels (every
     * 8-corner lookup of the plain volume then costs four 64-byte sectors).  Same values bit for bit.  Every other consumer
     * (adfp_sample_tsdf, the backward's TSDF gradient) reads `data`. */
    const float* corner_blocks;
} adfp_tsdf;

/* Everything DF.forward reads besides the points: decoder.py:307-353. */
typedef struct adfp_scene {
    double bound[3][2];       /* Renderer.bound / MLP.bound   (src/DF_Prior.py:177-194), f64 */
    double tsdf_bnds[3][2];   /* tsdf_bnds                    (src/DF_Prior.py:86-91),   f64 */
    adfp_grid low, high, color;
    adfp_tsdf tsdf;
    const float* w_low;       /* packed images (adfp_pack_decoder / adfp_pack_attention) */
    const float* w_high;
    const float* w_color;
    const float* w_att;
    /* optional "H" images (adfp_pack_decoder_h): when non-NULL the FORWARD decoders run their MLP on
     * f16 MFMA with a 3-product split of every f32 operand (fp32-grade accuracy);
     * NULL = exact f32-input MFMA from w_*. */
    const void* h_low;
    const void* h_high;
    const void* h_color;
    const void* h_att;        /* adfp_pack_attention_h */
    /* optional "T" images (adfp_pack_decoder_ht: the transposed weights as f16 hi/lo halves).  With them, and with the ReLU
     * masks the training forward left in adfp_train_state, the decoder BACKWARD runs on f16 MFMA with the same 3-product
     * split and recomputes nothing; NULL (or no masks, or a ray / point gradient requested) = the exact f32 backward from
     * w_*. */
    const void* ht_low;
    const void* ht_high;
    const void* ht_color;
    const void* ht_att;       /* adfp_pack_attention_ht: the attention network's backward on f16 MFMA */
    /* Flat (state_dict order) parameters of the four networks, optional.  With them, a forward call whose f16-split kernels
     * met an operand outside the f16 range (|x| >= 65504: a weight, a grid feature or a hidden activation) REPAIRS ITSELF: a
     * predicated fallback kernel re-evaluates the call's points in plain f32 from these buffers before anything consumes the
     * outputs (no host involvement, graph-capturable).  NULL = no repair; the call then only reports (status). */
    const float* flat_low;
    const float* flat_high;
    const float* flat_color;
    const float* flat_att;
    /* Sticky status word the kernels OR into (system-scope atomic): device memory or device-visible pinned host memory,
     * NULL = none.  ADFP_STATUS_F16_RANGE_<net>: the f16-split kernels of that network met an operand outside the f16 range
     * in some call since the caller last cleared the word.  With flat_* set that call's outputs were repaired (see above); the
     * caller should hand over the exact image (w_*, h_* = NULL) for that network from now on -- the repair is a slow path.
     * ADFP_STATUS_F16_RANGE_BWD: the same in a backward kernel (that call's gradients are not reliable). */
    int* status;
} adfp_scene;
#define ADFP_STATUS_F16_RANGE_LOW   1
#define ADFP_STATUS_F16_RANGE_HIGH  2
#define ADFP_STATUS_F16_RANGE_COLOR 4
#define ADFP_STATUS_F16_RANGE_ATT   8
#define ADFP_STATUS_F16_RANGE_BWD   16
#define ADFP_STATUS_F16_RANGE       31   /* any of them */
/* NOT a range bit, an ERROR: a wave of a persistent decoder kernel waited for a chunk of the chip-wide tile pool that was never
 * published (the counter block was not zero at launch, or a ring entry was overwritten early) and gave up after ~2^22 polls -- the
 * launch ended instead of hanging, tiles of that call were NOT computed.  The Python binding raises RuntimeError on it. */
#define ADFP_STATUS_POOL_TIMEOUT    32

typedef struct adfp_points {
    int mode;                 /* ADFP_PTS_* */
    long long n_points;       /* P (= n_rays * S in ray mode) */
    const void* pts;          /* [P,3] f64 or f32 (explicit modes) */
    const float* rays_o;      /* [N,3] (ray mode) */
    const float* rays_d;      /* [N,3] */
    const double* z_vals;     /* [N,S] */
    int S;
} adfp_points;

/* ---- info ------------------------------------------------------------------------- */
int adfp_version(void);
/* number of floats of the flat parameter buffer / of the packed image for a decoder kind */
long long adfp_decoder_flat_floats(int kind);
long long adfp_decoder_packed_floats(int kind);
long long adfp_attention_flat_floats(void);
long long adfp_attention_packed_floats(void);
/* bytes of scratch adfp_render_forward / adfp_eval_points need for P points */
size_t adfp_workspace_bytes(long long n_points);

/* ---- layout conversion -------------------------------------------------------------- */
/* [1,32,Z,Y,X] -> [Z,Y,X,32]  (and back, for gradients).  C must be 32. */
int adfp_relayout_grid(const float* src_cm, float* dst_cl, int C, int Z, int Y, int X, void* stream);
int adfp_relayout_grid_back(const float* src_cl, float* dst_cm, int C, int Z, int Y, int X, void* stream);
/* Several grids in ONE launch (a launch costs ~5 us of host time and ~5 us on the device whatever it converts; the Mapper
 * re-materialises three grids per iteration, src/Mapper.py:382-388).  back = 0: [32][V] -> [V][32]; back = 1: the way back.
 * At most ADFP_RELAYOUT_MAX_JOBS jobs; adfp_render_args.relayout_jobs hands the forward conversions to the render call itself. */
typedef struct adfp_relayout_job { const float* src; float* dst; long long voxels; } adfp_relayout_job;
#define ADFP_RELAYOUT_MAX_JOBS 4
int adfp_relayout_grids(int n_jobs, const adfp_relayout_job* jobs /*host*/, int back, void* stream);
/* TSDF volume (any strides; the reference's permuted view of get_tsdf.py:95-97 as it stands) -> its corner-block copy
 * dst[X][Y][Z][8] (8 X Y Z floats, z fastest): block (x, y, z) = the eight values a trilinear lookup with lower corner (x, y, z)
 * blends, v(min(x+dx, X-1), min(y+dy, Y-1), min(z+dz, Z-1)) at index dx + 2 dy + 4 dz.  Built once per volume (the TSDF is
 * static for a run); adfp_tsdf.corner_blocks hands it to the render path.  tsdf->corner_blocks is ignored here. */
int adfp_relayout_tsdf(const adfp_tsdf* tsdf /*host*/, float* dst, void* stream);
/* flat state_dict-order parameters -> packed MFMA image (MLP: decoder.py:91-203) */
int adfp_pack_decoder(int kind, const float* flat, float* packed, void* stream);
/* same parameters -> "H" image (f16 hi/lo halves of every weight), adfp_decoder_packed_h_words(kind) 32-bit words.
 * status (may be NULL): as adfp_scene.status -- ADFP_STATUS_F16_RANGE is raised for a weight with |w| >= 65504.
 * There is ONE pack kernel for the f16-split images (H, G, HT), adfp_pack_images' below; the five single-image entries
 * adfp_pack_decoder_h / _ht, adfp_pack_attention_h / _ht and adfp_pack_split_image are wrappers that hand it a one- or two-job
 * table (same arguments refused, same images, same status reporting as a job of adfp_pack_images). */
long long adfp_decoder_packed_h_words(int kind);
int adfp_pack_decoder_h(int kind, const float* flat, void* packed, int* status, void* stream);
/* -> "T" image for the f16-split backward, adfp_decoder_packed_ht_words(kind) 32-bit words */
long long adfp_decoder_packed_ht_words(int kind);
int adfp_pack_decoder_ht(int kind, const float* flat, void* packed, int* status, void* stream);
long long adfp_attention_packed_h_words(void);
long long adfp_attention_packed_ht_words(void);
int adfp_pack_attention_ht(const float* flat, void* packed, int* status, void* stream);
int adfp_pack_attention_h(const float* flat, void* packed, int* status, void* stream);
/* A split image holds TWO operand layouts back to back: H (v_mfma_f32_32x32x16_f16 order: the training forward, the
 * single-network entries) and G (v_mfma_f32_16x16x32_f16 order: the inference kernels).  adfp_pack_decoder_h / adfp_pack_attention_h
 * write both; this entry writes the chosen part(s) of the same buffer, so that a training iteration re-packs only the H part of
 * a trained network and an inference frame only the G part.  net: ADFP_DEC_LOW / _HIGH / _COLOR or ADFP_NET_ATT; which: bit 0 = H,
 * bit 1 = G.  A consumer must only be handed an image whose part IT reads is current:
 *   H: the high decoder / attention MLP of a training call (adfp_*_train with a state) whose state carries masks_<net>; the low or
 *      the colour decoder whenever it does NOT run inside the fused low + colour launch (stages low / high; the other one on its
 *      exact image; a training state with masks for one of the two only); adfp_decode_single / adfp_attention_rows; (the f16-split
 *      backward reads the separate ht images)
 *   G: the fused low + colour launch = stage colour with both networks on split images, inference or a training state that
 *      carries masks_low AND masks_color; the high decoder / attention MLP of an inference call or of a training call without
 *      masks_<net> (forward = the inference kernel, backward recomputes) */
#define ADFP_NET_ATT 3
#define ADFP_IMAGE_H 1
#define ADFP_IMAGE_G 2
int adfp_pack_split_image(int net, int which, const float* flat, void* packed, int* status, void* stream);
/* Several packed images in ONE launch (a Mapper iteration re-packs four per step: the trained networks' forward parts and their
 * transposed images): job = one image of one network.  format is exactly one of ADFP_IMAGE_H / ADFP_IMAGE_G (that part of the
 * split image buffer `packed`, as adfp_pack_split_image writes it) or ADFP_IMAGE_HT (`packed` = the transposed image of
 * adfp_pack_decoder_ht / adfp_pack_attention_ht).  The same kernel as those entries run, the same status reporting; at most
 * ADFP_PACK_MAX_JOBS jobs.  A render call's adfp_render_args.pack_jobs run the same code inside the call's first launch. */
#define ADFP_IMAGE_HT 4
#define ADFP_PACK_MAX_JOBS 8
typedef struct adfp_pack_job { int net; int format; const float* flat; void* packed; } adfp_pack_job;
int adfp_pack_images(int n_jobs, const adfp_pack_job* jobs /*host*/, int* status, void* stream);
/* mlp_tsdf parameters (decoder.py:206-258) */
int adfp_pack_attention(const float* flat, float* packed, void* stream);

/* ---- a1: get_rays (src/common.py:254-272) ------------------------------------------- */
/* c2w: [4,4] row-major fp32 on device (only the top 3 rows are read). */
int adfp_get_rays(int H, int W, float fx, float fy, float cx, float cy, const float* c2w,
                  float* rays_o /*[H*W,3]*/, float* rays_d /*[H*W,3]*/, void* stream);

/* ---- a2: get_rays_from_uv (src/common.py:76-91) ----------------------------------------- */
/* Rays through n pixels (pix_i = column, pix_j = row coordinates as float, as get_sample_uv hands them on); c2w [4,4]
 * row-major fp32 on the device.  The backward gives d/d c2w [4,4] (bottom row zero) from the cotangents of the rays:
 * the camera pose of the Tracker and of the Mapper's bundle adjustment reaches the renderer only through this function
 * (src/Tracker.py:97, src/Mapper.py:425).  Either cotangent may be NULL. */
int adfp_rays_from_uv(const float* pix_i, const float* pix_j, int n, float fx, float fy, float cx, float cy, const float* c2w,
                      float* rays_o /*[n,3]*/, float* rays_d /*[n,3]*/, void* stream);
int adfp_rays_from_uv_backward(const float* pix_i, const float* pix_j, int n, float fx, float fy, float cx, float cy,
                               const float* g_rays_o, const float* g_rays_d, float* g_c2w /*[4,4]*/, void* stream);

/* ---- a3: the Mapper's bounding-box pre-filter (src/Mapper.py:438-449) ------------------ */
/* Keeps ray i iff min over axes of max over the two bound planes of (bound - o) / d >= gt_depth
 * (f64 arithmetic on f32 rays, as the reference's f64 `self.bound` promotes it; NaN compares false).
 * bound_dev: [3][2] float64 ON THE DEVICE.  out_index [n_rays] int32 receives the kept ray ids in
 * ascending order (= boolean-mask indexing), *out_count (device int) their number. */
int adfp_prefilter_rays(const float* rays_o, const float* rays_d, const float* gt_depth, int n_rays,
                        const double* bound_dev, int* out_index, int* out_count, void* stream);

/* ---- a4: sampler (src/utils/Renderer.py:134-221) ------------------------------------ */
/* gt_depth may be NULL (then n_surface is ignored, near = 0.01).  t_rand [N,n_samples] is
 * the caller's torch.rand draw when perturb > 0 (Renderer.py:216), else NULL.
 * depth_max: optional device float holding max(gt_depth) over the FULL batch (used by the
 * multi-GPU path so that shards reproduce the single-GPU far clamp, Renderer.py:159/:195);
 * NULL = reduce it here.  scratch: >= 16 bytes of device memory. */
int adfp_sample_rays(const float* rays_o, const float* rays_d, const float* gt_depth, int n_rays,
                     const double bound[3][2], int n_samples, int n_surface, int lindisp,
                     float perturb, const float* t_rand, const float* depth_max,
                     double* z_vals /*[N, S]*/, void* scratch, void* stream);

/* ---- a5..a12: Renderer.eval_points + DF.forward (Renderer.py:27-71, decoder.py:307-353) */
/* raw [P,4] fp32 (rgb, occ), w [P] fp32 (attention weight).
 * flags & ADFP_EVAL_APPLY_BOUND: occ forced to 100 outside scene->bound (Renderer.py:51-64);
 * without it the call is DF.forward alone (what src/utils/Mesher.py:315 calls before applying
 * its own mask). */
#define ADFP_EVAL_APPLY_BOUND 1
int adfp_eval_points(const adfp_scene* scene /*host*/, const adfp_points* pts /*host*/, int stage, int flags,
                     float* raw, float* w, void* workspace, size_t workspace_bytes, void* stream);

/* The same with the state the point backward needs (autograd through Renderer.eval_points / DF.forward: the reference's
 * eval_points is autograd-transparent, src/utils/Renderer.py:27-71).  state = NULL is adfp_eval_points. */
struct adfp_train_state;
int adfp_eval_points_train(const adfp_scene* scene, const adfp_points* pts, int stage, int flags, float* raw, float* w,
                           void* workspace, size_t workspace_bytes, const struct adfp_train_state* state, void* stream);

/* a10 alone: Renderer.sample_grid_tsdf / eval_points_tsdf (Renderer.py:73-107) */
int adfp_sample_tsdf(const adfp_tsdf* tsdf /*host*/, const double tsdf_bnds[3][2],
                     const adfp_points* pts /*host*/, float* out /*[P]*/, void* stream);

/* ---- a13: raw2outputs_nerf_color, occupancy branch (src/common.py:206-251) ------------ */
/* weights may be NULL.  depth/uncertainty are float64 like the reference's. */
int adfp_composite(const float* raw /*[N,S,4]*/, const double* z_vals /*[N,S]*/, int n_rays, int S,
                   double* depth, double* uncertainty, float* color /*[N,3]*/,
                   float* weights /*[N,S] or NULL*/, void* stream);

/* Buffers the backward needs from the forward (training only).  Caller-owned, sized for P points:
 * flags P bytes, list P ints, counter >= 64 bytes (int[0] = length of the in-band list, int[8] = the forward call's f16-range
 * flag: non-zero = the forward was repaired by the f32 fallback, the ReLU masks / layer inputs it left are not valid, and the
 * backward entries then return ZERO gradients for that call -- see adfp_scene.flat_*), att_occ / att_u P floats.
 * Optional, for the f16-split backward (scene->h_* and ->ht_* set; any of them may be NULL = exact backward for that
 * decoder): masks_* = ADFP_TRAIN_MASK_WORDS 32-bit words per point, the ReLU masks of the decoder's five layers;
 * act_* = adfp_train_act_floats(kind) floats per point, the inputs of every layer (position, Fourier features, grid
 * features, h_0..h_4) -- only needed when that decoder's parameter gradient (g_flat_*) will be requested. */
#define ADFP_TRAIN_MASK_WORDS 6
typedef struct adfp_train_state {
    unsigned char* flags;
    int* list;
    int* counter;
    float* att_occ;
    float* att_u;
    unsigned* masks_low;
    unsigned* masks_high;
    unsigned* masks_color;
    float* act_low;
    float* act_high;
    float* act_color;
    unsigned* masks_att;      /* ADFP_TRAIN_ATT_MASK_WORDS words per point (in-band list entry): masks + softmax weights */
    float* act_att;           /* ADFP_TRAIN_ATT_ACT_FLOATS floats per point, only when g_flat_att will be requested */
    /* Debug export, optional (NULL = none), written by the BACKWARD entries: the ReLU decisions the EXACT backward kernels
     * recomputed for a network (they differentiate their own f32 forward, which decides a unit within rounding of zero on its
     * own), in the layout of masks_* / masks_att.  A network that took the f16-split backward used the forward's masks_* and
     * leaves its dbg buffer untouched.  With these a test differentiates the oracle along the SAME piecewise-linear function
     * (oracle/adfp_oracle.py: relu_masks) and holds every gradient element to the forward tolerance. */
    unsigned* dbg_masks_low;
    unsigned* dbg_masks_high;
    unsigned* dbg_masks_color;
    unsigned* dbg_masks_att;
} adfp_train_state;
#define ADFP_TRAIN_ATT_MASK_WORDS 14
#define ADFP_TRAIN_ATT_ACT_FLOATS 416
long long adfp_train_act_floats(int kind);

/* A call whose rays ARE consecutive pixels of one camera frame (Renderer.render_img, src/utils/Renderer.py:278-327, and a rank's
 * contiguous share of it): the call's FIRST launch -- the one that zeroes its device words and packs the weight images it was
 * handed -- also writes the rays of pixels [first, first + n_rays) (src/common.py:254-272, adfp_get_rays' arithmetic) and reduces
 * max(gt_depth) of every ray_batch_size segment of the WHOLE frame (src/utils/Renderer.py:294-313 with :159, :195).  A ray shard
 * then costs no launch for "the rays of the frame" and none for "the maxima of rays it does not hold".
 * `first` = adfp_render_args.depth_max_first_ray; the segment length = depth_max_segment (> 0 required; depth_max must be NULL). */
typedef struct adfp_frame_job {
    const float* c2w;           /* device float[16] (row-major 4x4; rows 0-2 are read): camera-to-world */
    int H, W;
    float fx, fy, cx, cy;
    const float* depth;         /* device float[H*W]: the whole frame's sensor depth; the call's gt_depth = depth + first */
    float* rays_o;              /* [n_rays,3] OUT (caller-owned; the kernels after the first launch read them) */
    float* rays_d;              /* [n_rays,3] OUT */
} adfp_frame_job;

/* ---- a4..a13 in one call: Renderer.render_batch_ray (Renderer.py:110-255) ------------- */
typedef struct adfp_render_args {
    int stage;
    int n_rays;
    int n_samples, n_surface;   /* cfg['rendering'] (configs/df_prior.yaml:93-98) */
    int lindisp;
    float perturb;
    const float* rays_o;        /* [N,3] */
    const float* rays_d;        /* [N,3] */
    const float* gt_depth;      /* [N] or NULL */
    const float* t_rand;        /* [N,n_samples] or NULL */
    const float* depth_max;     /* device float or NULL */
    double* depth;              /* [N]   out */
    double* uncertainty;        /* [N]   out */
    float* color;               /* [N,3] out */
    float* weight;              /* [N,S] out: attention weight (decoder.py:333) */
    double* z_vals;             /* [N,S] out, optional (NULL = keep in workspace) */
    float* raw;                 /* [N,S,4] out, optional */
    void* workspace;
    size_t workspace_bytes;
    const adfp_train_state* state;  /* NULL for inference; else the forward leaves its state here */
    /* > 0: the call's rays are consecutive SEGMENTS of this many rays, each with its own max(gt_depth) for the far clamp and the
     * zero-depth surface range -- what Renderer.render_img's ray batches have (src/utils/Renderer.py:294-313: every 100 000-ray
     * batch clamps `far` with its own maximum) -- so that a whole frame is ONE call with the batched loop's results bit for bit.
     * depth_max, when given, then holds one float per segment; otherwise the maxima are reduced here (at most 48 segments).
     * 0: one maximum for the whole call (render_batch_ray). */
    int depth_max_segment;
    /* With depth_max_segment > 0 and depth_max given: the index, in the segmented batch, of this call's FIRST ray -- the call is a
     * ray shard [first, first + n_rays) of a frame (one GPU's share, attentive_dfprior_amd.dist.render_img_sharded), ray i belongs
     * to segment (first + i) / depth_max_segment, and depth_max holds the maxima of the WHOLE frame's segments.  0 otherwise
     * (non-zero without depth_max or `frame` is ADFP_E_ARG: the call cannot know the maxima of rays it does not hold). */
    int depth_max_first_ray;
    /* Optional: weight images this call's kernels read and that are not packed yet (adfp_pack_images' jobs, host array, at most
     * ADFP_PACK_MAX_JOBS) -- packed by the call's FIRST launch, beside the zero fill of its device words (two launches of ~5 us
     * inside a graph replay otherwise; a Mapper iteration re-packs the trained networks' images every step).  A weight outside
     * the f16 range is reported to scene->status as by adfp_pack_images.  NULL / 0: none. */
    const adfp_pack_job* pack_jobs;
    int n_pack_jobs;
    /* Optional (host struct, NULL = none): the call renders pixels [depth_max_first_ray, + n_rays) of this frame; rays_o / rays_d /
     * gt_depth above are then ignored (the rays are written to frame->rays_o / rays_d, gt_depth = frame->depth + first). */
    const adfp_frame_job* frame;
    /* Optional: feature grids this call's kernels read in channels-last form and that are not converted yet (host array of
     * [32][V] -> [V][32] jobs, at most ADFP_RELAYOUT_MAX_JOBS): converted by extra workgroups of the call's SECOND launch (the
     * sampler: latency-bound, most of the chip idle) -- the decoders, the first readers, are two launches later.  NULL / 0: none. */
    const adfp_relayout_job* relayout_jobs;
    int n_relayout_jobs;
    /* Optional: the Mapper's bounding-box pre-filter (src/Mapper.py:438-449: keep a ray iff min_axis max_side((bound - o) / d) >=
     * gt_depth, in float64) as a job of the call's first launch instead of a launch of its own (adfp_prefilter_mask): that launch
     * writes prefilter_keep[ray] (1 / 0) for every ray of the call, and the call's far clamp is max(gt_depth) over the KEPT rays
     * (adfp_prefilter_mask's depth_max).  All rays are rendered; the caller masks the dropped ones out of loss and gradients
     * (adfp_loss_args.keep, adfp_backward_args.ray_keep).  prefilter_bound: device double[6] = (lo, hi) per axis.  Needs gt_depth,
     * no depth_max, depth_max_segment = 0, no frame.  NULL: none. */
    const double* prefilter_bound;
    unsigned char* prefilter_keep;
} adfp_render_args;

int adfp_render_forward(const adfp_scene* scene /*host*/, const adfp_render_args* args /*host*/, void* stream);

/* ---- a15: backward of render_batch_ray (autograd of src/Mapper.py:457-473) -------------- */
/* Cotangents of (depth, uncertainty, color, weight) -> gradients of the three feature grids
 * (channels-last, converted back by adfp_relayout_grid_back) and of the decoder parameters (flat
 * state_dict order).  Any output pointer may be NULL (= not needed: frozen decoder, lr 0 grid).
 * z_vals, raw and `state` are the ones the forward call wrote.  Every non-NULL output is zeroed and then accumulated:
 * the grid gradients with float atomics (not bitwise reproducible run to run), the parameter gradients atomic-free through
 * per-workgroup partial sums (reproducible).
 * Two implementations per decoder, chosen by what the caller provides: with scene->ht_* and the forward's state->masks_* (and
 * state->act_* when g_flat_* is wanted) the f16-split backward (f16 MFMA, nothing recomputed, grid gradients scattered in
 * sorted order); otherwise -- and always when g_rays_* / g_pts is requested -- the exact f32 backward from scene->w_*.  The
 * attention network likewise (ht_att + state->masks_att [+ act_att], else w_att).
 * g_rays_o / g_rays_d: gradients w.r.t. the rays (p = o + d z; through the trilinear coordinates of the
 * feature grids and the TSDF and through sin(p @ B)) for the Tracker, src/Tracker.py:112-133. */
typedef struct adfp_backward_args {
    int stage;
    int n_rays;
    int S;                       /* samples per ray of the forward call */
    const float* rays_o;
    const float* rays_d;
    const double* z_vals;        /* [N,S] from the forward */
    const float* raw;            /* [N,S,4] from the forward */
    adfp_train_state state;
    const double* g_depth;       /* [N] or NULL */
    const double* g_uncertainty; /* [N] or NULL */
    const float* g_color;        /* [N,3] or NULL */
    const float* g_weight;       /* [N,S] or NULL */
    float* g_grid_low;           /* [Z,Y,X,32] channels-last, or NULL */
    float* g_grid_high;
    float* g_grid_color;
    float* g_flat_low;           /* adfp_decoder_flat_floats(kind) floats, or NULL */
    float* g_flat_high;
    float* g_flat_color;
    float* g_flat_att;           /* adfp_attention_flat_floats() floats, or NULL */
    float* g_rays_o;             /* [N,3] or NULL: camera tracking (src/Tracker.py:112-133) */
    float* g_rays_d;             /* [N,3] or NULL */
    void* workspace;
    size_t workspace_bytes;
    const unsigned char* ray_keep;  /* [N] or NULL: rays flagged 0 (adfp_prefilter_mask) receive no gradient at all */
    int options;                 /* ADFP_BWD_* bits, 0 = defaults */
    /* Optional second lane (NULL = none: everything runs on `stream`, in order).  The spatial sort of the sample points -- nine
     * short, latency-bound launches whose result only k_scatter_sorted, the call's LAST launch, reads -- then runs on
     * `side_stream` BESIDE the backward kernels instead of in front of them: the call records side_events[0] on `stream` when the
     * sort keys exist, makes `side_stream` wait for it and sorts there; before the scatter it records side_events[1] on the lane
     * and makes `stream` wait for it.  While the lane is busy the call's persistent kernels (a whole CU per workgroup) leave
     * ADFP_SIDE_CU_RESERVE compute units free, or the lane's launches would each wait for a whole kernel to retire.  On return
     * `stream` has joined the lane: work queued on `stream` afterwards is ordered after everything, also inside a stream capture
     * (fork and join are captured as graph dependencies).  Caller-owned: a hipStream_t of the same device and two hipEvent_t
     * (timing disabled is fine) that no other call in flight uses. */
    void* side_stream;
    void* side_events[2];
} adfp_backward_args;
/* grid gradients of the f16-split backward through the in-kernel write-combining scatter instead of the sorted scatter
 * (k_bin_keys + radix sort + k_scatter_sorted); same values up to the order of the float atomics */
#define ADFP_BWD_SCATTER_IN_KERNEL 1
/* the caller guarantees that the g_grid_* buffers are all zero on entry (adfp_adam_grids_cl leaves them so): the call does not
 * zero them again */
#define ADFP_BWD_GRIDS_PREZEROED 2
/* weight gradients of the 32-channel decoders through the staged two-kernel path (cotangent blocks written per point, k_outer_h)
 * instead of inside the chain kernel (k_decode_bwd_fused); same values up to the summation order.  What the tests compare the
 * fused kernel against. */
#define ADFP_BWD_STAGED_WGRAD 4
/* weight gradients inside the chain kernel, but with round 3-4's one-wave-per-SIMD kernel (k_decode_bwd_fused: every wave keeps
 * all sixteen gradient blocks) instead of the role-split kernel at two waves per SIMD (k_decode_bwd_roles).  A/B runs. */
#define ADFP_BWD_FUSED_ONE_WAVE 8
size_t adfp_backward_workspace_bytes(long long n_points);
int adfp_render_backward(const adfp_scene* scene /*host*/, const adfp_backward_args* args /*host*/, void* stream);

/* Backward of adfp_eval_points_train: cotangents of raw [P,4] and of the attention weight [P] -> gradients of the grids and
 * decoder parameters (as adfp_render_backward) and of the query points themselves (g_pts [P,3] fp32; through the trilinear
 * coordinates of the feature grids and of the TSDF and through sin(p @ B)).  With ADFP_EVAL_APPLY_BOUND in `flags`, points outside
 * scene->bound pass no occupancy gradient (the forward overwrote their occupancy with 100).  Any output may be NULL. */
typedef struct adfp_points_backward_args {
    int stage;
    int flags;                   /* ADFP_EVAL_* of the forward call */
    adfp_train_state state;      /* the one the forward call filled */
    const float* g_raw;          /* [P,4] or NULL */
    const float* g_w;            /* [P] or NULL */
    float* g_grid_low;           /* [Z,Y,X,32] channels-last, or NULL */
    float* g_grid_high;
    float* g_grid_color;
    float* g_flat_low;           /* adfp_decoder_flat_floats(kind) floats, or NULL */
    float* g_flat_high;
    float* g_flat_color;
    float* g_flat_att;
    float* g_pts;                /* [P,3] or NULL */
    void* workspace;             /* adfp_backward_workspace_bytes(P) */
    size_t workspace_bytes;
    int options;                 /* ADFP_BWD_* bits, 0 = defaults */
} adfp_points_backward_args;
int adfp_eval_points_backward(const adfp_scene* scene /*host*/, const adfp_points* pts /*host*/, const adfp_points_backward_args* args /*host*/,
                              void* stream);

/* ---- TSDF fusion of one RGB-D frame (src/fusion.py:69-142 CUDA kernel, launch :226-251) ---- */
/* tsdf / weight / color: device volumes in the reference's physical order [X][Y][Z] (Z fastest), updated in
 * place; color may be NULL.  origin, cam_intr (3x3) and cam_pose (4x4 camera-to-world, already in the
 * OpenCV convention of get_tsdf.py:79-80) are HOST arrays; color_im is the packed b*65536+g*256+r image
 * (src/fusion.py:223), depth_im the depth image, both [H,W] fp32 on the device. */
int adfp_tsdf_integrate(float* tsdf, float* weight, float* color, int dim_x, int dim_y, int dim_z, const float origin[3],
                        float voxel_size, const float cam_intr[9], const float cam_pose[16], const float* color_im,
                        const float* depth_im, int im_h, int im_w, float trunc_margin, float obs_weight, void* stream);

/* ---- Mapper bookkeeping on the device ----------------------------------- */
/* Frustum feature selection, src/Mapper.py:90-158: which points of an X x Y x Z feature grid (point
 * coordinates = linspace over `bound` per axis) project into the current depth image in front of the sensed
 * surface (+0.5 m), plus the ball of radius 0.5 m around the camera centre.  The reference does this on the
 * host with numpy and cv2.remap (bilinear, 1/32-pixel map rounding, constant-0 border -- restated here).
 * c2w / w2c (= inverse, computed by the caller) are HOST 4x4 row-major fp32; depth is the [H,W] fp32 image on
 * the device; sampled: X*Y*Z floats of device workspace; scratch: 4 bytes of device workspace.
 * mask: X*Y*Z bytes written in the grid tensor's [Z][Y][X] order (the permute(2,1,0) of src/Mapper.py:345). */
int adfp_frustum_mask(int X, int Y, int Z, const double bound[3][2], const float c2w[16], const float w2c[16],
                      double fx, double fy, double cx, double cy, int H, int W, const float* depth,
                      float* sampled, unsigned* scratch, unsigned char* mask, void* stream);
/* One torch.optim.Adam step (amsgrad off, weight_decay 0; src/Mapper.py:374-378, :473) on the masked
 * voxels of a channel-major grid [channels][nvox], in place -- instead of the reference's compact copy
 * `val[mask]` that is index_put into the grid before and after every iteration (src/Mapper.py:347-361,
 * :382-388, :476-482).  exp_avg / exp_avg_sq have the grid's shape and must be zero before step 1; elements
 * outside the mask (mask == NULL: none) are not touched.  step counts from 1. */
int adfp_masked_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const unsigned char* mask,
                     long long nvox, int channels, float lr, float beta1, float beta2, float eps, int step, void* stream);

/* ---- One Mapper iteration as a fixed, sync-free kernel sequence (src/Mapper.py:438-473) ------------------------------- */
/* The bounding-box pre-filter of adfp_prefilter_rays as a per-ray keep flag (1 = kept) plus *depth_max = the max sensor
 * depth of the KEPT rays (device float, feeds adfp_render_args.depth_max).  The reference compacts the batch with boolean
 * indexing (a device sync, a data-dependent batch size); rendering the dropped rays too and masking them out of the loss
 * (adfp_loss_args.keep, adfp_backward_args.ray_keep) gives the kept rays identical outputs and gradients, because a ray
 * sees the rest of its batch only through max(gt_depth) (src/utils/Renderer.py:159, :195). */
int adfp_prefilter_mask(const float* rays_o, const float* rays_d, const float* gt_depth, int n_rays, const double* bound_dev,
                        unsigned char* keep /*[N]*/, float* depth_max /*device float*/, void* stream);
/* The Mapper's loss (src/Mapper.py:457-469) and its cotangents w.r.t. the renderer's outputs:
 *   sum_{gt_depth > 0} |gt_depth - depth|  [+ sum |weight - 1| when `warmup`]  [+ w_color_loss * sum |gt_color - color| in stage color]
 * g_* = d loss / d output (sign functions, 0 at 0 like torch.abs's backward), zero for rays with keep == 0.
 * loss (device double, REQUIRED: a NULL loss is ADFP_E_ARG) is ACCUMULATED by adfp_mapper_loss: zero it first. */
typedef struct adfp_loss_args {
    int n_rays, S;
    int stage;                   /* ADFP_STAGE_*; the colour term exists in stage color only */
    int warmup;                  /* src/Mapper.py:459: idx <= 1 and the 5 iterations after the low stage */
    float w_color_loss;          /* configs/df_prior.yaml:56 */
    const double* depth;         /* [N]   */
    const float* color;          /* [N,3] (stage color) */
    const float* weight;         /* [N,S] attention weight (warm-up) */
    const float* gt_depth;       /* [N]   */
    const float* gt_color;       /* [N,3] (stage color) */
    const unsigned char* keep;   /* [N] or NULL */
    double* loss;                /* device double, required */
    double* g_depth;             /* [N]   out */
    float* g_color;              /* [N,3] out (stage color; may be NULL otherwise) */
    float* g_weight;             /* [N,S] out (warm-up; may be NULL otherwise) */
} adfp_loss_args;
int adfp_mapper_loss(const adfp_loss_args* args /*host*/, void* stream);
/* The same kernel doing three launches' work (inside a graph replay a launch costs ~5 us whatever it does):
 *  - the loss is WRITTEN, not accumulated (no zero fill first): per-workgroup partial sums go to scratch + 8 and the workgroup
 *    that draws the last ticket adds them up in order (reproducible, unlike the atomics of adfp_mapper_loss).  scratch: device
 *    memory, 8-byte aligned, adfp_mapper_loss_scratch_bytes(n_rays) bytes, whose first int is ZERO before the first call (the
 *    kernel leaves it zero);
 *  - adfp_adam_prep's work (below: same arguments, n_groups may be 0) is done by the first workgroup on the side.
 * With n_rays == 0 nothing is launched: zero the loss and call adfp_adam_prep yourself. */
size_t adfp_mapper_loss_scratch_bytes(int n_rays);
int adfp_mapper_loss_step(const adfp_loss_args* args /*host*/, void* scratch, size_t scratch_bytes, int* steps, float* derived, int n_groups,
                          const float* lr /*host*/, float beta1, float beta2, const int* skip_flag, void* stream);
/* torch.optim.Adam's step counters and bias corrections on the device, for n_groups <= 8 parameter groups in ONE launch:
 * for every group g with lr[g] >= 0:  steps[g] += 1,  derived[2g] = lr[g] / (1 - beta1^steps[g]),  derived[2g+1] =
 * sqrt(1 - beta2^steps[g])  (double arithmetic, one rounding, like the python floats of torch.optim); a negative lr[g]
 * = the group has no gradient in this iteration and does not step.  lr is a HOST array. */
/* skip_flag (device int, may be NULL): when *skip_flag != 0 at run time no group steps and `derived` is zeroed, which makes
 * adfp_masked_adam_dev / _multi leave parameters and moments untouched -- the Mapper iteration hands over the forward call's
 * f16-range flag (adfp_train_state.counter + 8) so that an iteration whose gradients are not valid changes nothing. */
int adfp_adam_prep(int* steps /*device int[n]*/, float* derived /*device float[n][2]*/, int n_groups, const float* lr /*host*/,
                   float beta1, float beta2, const int* skip_flag, void* stream);
/* adfp_masked_adam with the step-dependent scalars read from `derived`: no host value changes from step to step, so
 * the call can be replayed from a HIP graph. */
int adfp_masked_adam_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const unsigned char* mask,
                         long long nvox, int channels, float beta1, float beta2, float eps, const float* derived, void* stream);
/* The same for up to 8 parameter groups in ONE launch (a Mapper iteration steps three grids and two networks). */
typedef struct adfp_adam_group {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
    const unsigned char* mask;   /* [nvox] or NULL */
    long long nvox; int channels;
    const float* derived;        /* this group's {step size, sqrt(bias correction 2)} from adfp_adam_prep */
} adfp_adam_group;
int adfp_masked_adam_multi(int n_groups, const adfp_adam_group* groups /*host*/, float beta1, float beta2, float eps, void* stream);
/* The same step on feature grids whose optimiser state lives in the KERNELS' layout: gradient (as adfp_render_backward writes it),
 * both moments and a shadow copy of the parameters are channels-last [nvox][32]; the reference-layout grid [32][nvox] that the
 * rest of the system sees (the Tracker reads it from another process, src/Tracker.py:144-147) is written through.  One launch
 * replaces, per grid and iteration, the forward's re-layout of the updated grid, the backward's re-layout of the gradient and
 * the zeroing of the gradient buffer: every gradient element is set to zero as it is consumed (masked or not), so the buffer
 * can go straight into the next adfp_render_backward with ADFP_BWD_GRIDS_PREZEROED.  A skipped step (derived == {0, 0},
 * adfp_adam_prep's skip_flag) still zeroes the gradient.  Up to 8 grids per launch. */
typedef struct adfp_adam_cl_group {
    float* param_cl;             /* [nvox][32] shadow of the grid the render kernels read */
    float* param_cm;             /* [32][nvox] the reference-layout grid, written through on the masked voxels */
    float* grad_cl;              /* [nvox][32], consumed and zeroed */
    float* exp_avg_cl; float* exp_avg_sq_cl;
    const unsigned char* mask;   /* [nvox] or NULL */
    long long nvox;
    const float* derived;        /* {step size, sqrt(bias correction 2)} from adfp_adam_prep */
} adfp_adam_cl_group;
int adfp_adam_grids_cl(int n_groups, const adfp_adam_cl_group* groups /*host*/, float beta1, float beta2, float eps, void* stream);
/* adfp_adam_grids_cl and adfp_masked_adam_multi in ONE launch: every parameter group a Mapper iteration steps (either list may be empty) */
int adfp_adam_step(int n_cl_groups, const adfp_adam_cl_group* cl_groups /*host*/, int n_groups, const adfp_adam_group* groups /*host*/,
                   float beta1, float beta2, float eps, void* stream);

/* ---- One Tracker iteration as a fixed, sync-free kernel sequence (src/Tracker.py:75-134) ---------------------------------- */
/* Camera tensor (quaternion r, i, j, k + translation, 7 floats ON THE DEVICE) -> camera-to-world [4,4] row-major, and the
 * cotangent of c2w (rows 0-2) -> the cotangent of the 7 parameters: get_camera_from_tensor / quad2rotation of
 * src/common.py:139-178 and their autograd.  The pose the Tracker optimises reaches the renderer only through these. */
int adfp_camera_from_tensor(const float* cam /*[7] device*/, float* c2w /*[16] device*/, void* stream);
int adfp_camera_from_tensor_backward(const float* cam, const float* g_c2w /*[16]*/, float* g_cam /*[7]*/, void* stream);
/* The n sampled pixels of get_sample_uv (src/common.py:94-124): idx[t] indexes the window [H0,H1) x [W0,W1) in row-major
 * order (the caller's ONE torch.randint draw); out: pixel coordinates as floats (pix_i = column, pix_j = row, what
 * adfp_rays_from_uv takes), sensor depth [n] and colour [n,3] gathered from the [H,W] / [H,W,3] fp32 images. */
int adfp_select_pixels(const long long* idx /*[n] int64 device*/, int n, int H0, int H1, int W0, int W1, int H, int W,
                       const float* depth_img, const float* color_img, float* pix_i, float* pix_j, float* gt_depth, float* gt_color,
                       void* stream);
/* The Mapper's ray batch of one iteration (src/Mapper.py:421-436: get_samples per keyframe of the optimisation window, then four
 * torch.cat) in ONE launch: frame f contributes n rays -- pixel idx[t] of the window like adfp_select_pixels, its ray like
 * adfp_rays_from_uv (bit for bit), sensor depth and colour -- at rows [f n, f n + n) of the outputs.  The draws stay the caller's (one
 * torch.randint per frame: the reference's index stream).  c2w: device [4,4] row-major fp32, or NULL and the pose in c2w_host (rows
 * 0-2 of the matrix, row-major).  No gradient towards the poses (bundle adjustment takes adfp_ba_head / adfp_ba_tail). */
#define ADFP_KEYFRAMES_MAX 16
typedef struct adfp_keyframe {
    const long long* idx;      /* [n] int64, device */
    const float* c2w;          /* device, or NULL */
    float c2w_host[12];
    const float* depth_img;    /* [H,W] fp32 */
    const float* color_img;    /* [H,W,3] fp32 */
} adfp_keyframe;
int adfp_sample_keyframes(int n_frames, const adfp_keyframe* frames /*host*/, int n, int H0, int H1, int W0, int W1, int H, int W,
                          float fx, float fy, float cx, float cy, float* rays_o /*[n_frames n,3]*/, float* rays_d, float* gt_depth /*[n_frames n]*/,
                          float* gt_color /*[n_frames n,3]*/, void* stream);
/* The head and the tail of a Tracker iteration as ONE launch each (a launch costs ~5 us inside a graph replay whatever it does, and
 * the chain below is seven of them).
 * adfp_tracker_head = adfp_camera_from_tensor + adfp_select_pixels + adfp_rays_from_uv + adfp_prefilter_mask, same arithmetic:
 *   cam [7] -> c2w [16]; the n drawn pixels -> pix_i / pix_j / gt_depth / gt_color, their rays, the bounding-box keep flags and
 *   the largest sensor depth of the kept rays.
 * adfp_tracker_tail = adfp_rays_from_uv_backward + adfp_camera_from_tensor_backward [+ adfp_adam_prep + adfp_masked_adam_multi on
 *   the pose's parameter groups + adfp_track_keep_best]: ray cotangents -> g_c2w [16] -> g_cam [7]; with step != 0 the Adam step of
 *   torch.optim.Adam on cam (groups: n_groups = 1 -> the 7 parameters with lr[0]; 2 -> translation cam[4..7) with lr[0], quaternion
 *   cam[0..4) with lr[1], src/Tracker.py:219-229) and the running best pose -- kept BEFORE the step when n_groups = 2, after it
 *   when n_groups = 1 (the reference rebuilds / clones its camera tensor at those points, src/Tracker.py:236-263).  steps [n_groups]
 *   int / derived [n_groups][2] float as adfp_adam_prep; skip_flag as there. */
typedef struct adfp_tracker_head_args {
    const float* cam; float* c2w;
    const long long* idx; int n; int H0, H1, W0, W1, H, W;
    const float* depth_img; const float* color_img;
    float fx, fy, cx, cy;
    const double* bound;                     /* device [6] */
    float* pix_i; float* pix_j; float* gt_depth; float* gt_color; float* rays_o; float* rays_d;
    unsigned char* keep; float* depth_max;
} adfp_tracker_head_args;
int adfp_tracker_head(const adfp_tracker_head_args* args /*host*/, void* stream);
typedef struct adfp_tracker_tail_args {
    const float* pix_i; const float* pix_j; int n; float fx, fy, cx, cy;
    const float* g_rays_o; const float* g_rays_d;
    float* cam; float* g_c2w; float* g_cam;
    int step;                                /* 0: gradients only */
    float* exp_avg; float* exp_avg_sq;       /* [7] each */
    int* steps; float* derived; int n_groups; float lr[2]; float beta1, beta2, eps; const int* skip_flag;
    const double* loss; double* best_loss; float* best_cam;
} adfp_tracker_tail_args;
int adfp_tracker_tail(const adfp_tracker_tail_args* args /*host*/, void* stream);
/* ---- The Mapper's bundle adjustment: the window's poses as parameters of the Mapper's Adam ------------------------------------ */
/* The reference dropped this code (a `camera_tensor_id = 0` is left at src/Mapper.py:413); its parent project runs it under
 * mapping.BA.  Three launches around the fused Mapper iteration, for 1 <= n_frames <= ADFP_KEYFRAMES_MAX window frames with n >= 1
 * rays each; frame f owns rows [f n, f n + n) of every per-ray array and row f of cam [F,7] / c2w [F,16] / g_c2w [F,16] / g_cam [F,7].
 * A frame is FREE (its pose is the camera tensor cam[f], quaternion first, then translation) or FIXED (the gauge: its stored
 * matrix is used verbatim).
 * adfp_ba_head = adfp_camera_from_tensor per free frame + adfp_sample_keyframes over the window, bit for bit: c2w[f] (a fixed frame's
 *   is a copy of its stored [4,4]), and per ray pix_i / pix_j (what the tail takes), rays_o / rays_d, gt_depth, gt_color.
 * adfp_ba_tail = per frame adfp_rays_from_uv_backward on its rows + adfp_camera_from_tensor_backward, bit for bit (one workgroup per
 *   frame with adfp_tracker_tail's partition and summation order: reproducible), then with step != 0 the Adam update of the frame's
 *   7 parameters with the pose group's `derived` = {step size, sqrt(bias correction 2)} as adfp_adam_prep / adfp_mapper_loss_step
 *   leave them ({0, 0} = that iteration is skipped; skip_flag, optional, as there).  A fixed frame gets g_c2w = g_cam = 0; its
 *   tensor and moments are not touched.
 * adfp_cameras_from_tensors: cam[f] -> the 16 floats at dst[f] for every f with dst[f] != NULL (dst: HOST array of n_frames device
 *   pointers) -- the write-back of the optimised poses into their keyframe rows.
 * Errors, before any launch: ADFP_E_ARG for a NULL pointer (a fixed frame's c2w included; a free frame's may be NULL), n_frames
 * outside [1, ADFP_KEYFRAMES_MAX], n < 1, a pixel window outside the image; ADFP_E_UNSUPPORTED beyond 2^29 rays. */
typedef struct adfp_ba_frame {
    const long long* idx;      /* [n] int64 device: the frame's draw over the window [H0,H1) x [W0,W1), row-major */
    const float* c2w;          /* device [4,4]: the stored pose, read when free_pose == 0 */
    const float* depth_img;    /* [H,W] fp32 */
    const float* color_img;    /* [H,W,3] fp32 */
    int free_pose;
} adfp_ba_frame;
typedef struct adfp_ba_head_args {
    int n_frames, n; int H0, H1, W0, W1, H, W;
    float fx, fy, cx, cy;
    const float* cam; float* c2w;
    float* pix_i; float* pix_j; float* rays_o; float* rays_d; float* gt_depth; float* gt_color;
    adfp_ba_frame frames[ADFP_KEYFRAMES_MAX];
} adfp_ba_head_args;
int adfp_ba_head(const adfp_ba_head_args* args /*host*/, void* stream);
typedef struct adfp_ba_tail_args {
    int n_frames, n; float fx, fy, cx, cy;
    const float* pix_i; const float* pix_j; const float* g_rays_o; const float* g_rays_d;
    float* cam; float* g_c2w; float* g_cam;
    const unsigned char* free_flags;         /* device [F]: nonzero = frame f is free (device memory: a captured graph serves any gauge) */
    int step;                                /* 0: gradients only */
    float* exp_avg; float* exp_avg_sq;       /* [F,7] each */
    const float* derived;                    /* device [2], the pose group's */
    float beta1, beta2, eps; const int* skip_flag;
} adfp_ba_tail_args;
int adfp_ba_tail(const adfp_ba_tail_args* args /*host*/, void* stream);
int adfp_cameras_from_tensors(int n_frames, const float* cam /*[F,7] device*/, float* const* dst /*host [F]*/, void* stream);
/* The tracking loss (src/Tracker.py:115-129) and its cotangents:
 *   tmp = |gt_depth - depth| / sqrt(uncertainty + 1e-10)        (float64, uncertainty detached)
 *   mask = keep & (gt_depth > 0) [& tmp < 10 median(tmp over the kept rays) when handle_dynamic]
 *   loss = sum_mask tmp + w_color_loss sum_mask |gt_color - color|
 * torch.median's lower-middle element; at most 8192 rays (one workgroup).  loss (device double) is WRITTEN, not accumulated. */
typedef struct adfp_track_loss_args {
    int n_rays;
    int handle_dynamic;          /* configs/df_prior.yaml:28 */
    float w_color_loss;          /* :31 */
    const double* depth;         /* [N] */
    const double* uncertainty;   /* [N] */
    const float* color;          /* [N,3] */
    const float* gt_depth;       /* [N] */
    const float* gt_color;       /* [N,3] */
    const unsigned char* keep;   /* [N] or NULL: the bounding-box pre-filter of :100-109 as a keep flag (adfp_prefilter_mask) */
    double* loss;                /* device double or NULL */
    double* g_depth;             /* [N] out */
    float* g_color;              /* [N,3] out */
} adfp_track_loss_args;
int adfp_tracker_loss(const adfp_track_loss_args* args /*host*/, void* stream);
/* The iteration loop's running best (src/Tracker.py:261-263): if *loss < *best_loss then *best_loss = *loss and best_cam[0..7) =
 * cam[0..7); all four on the device, NaN never wins.  Start best_loss at +inf (the reference's 1e10). */
int adfp_track_keep_best(const double* loss, const float* cam, double* best_loss, float* best_cam, void* stream);

/* Stable radix sort of n (key, value) int pairs by the low key_bits bits of the (non-negative) keys, in place (key_tmp / val_tmp:
 * n ints each).  What the f16-split backward orders the sample points with (by grid cell, adfp_sort.h); exported for testing. */
size_t adfp_sort_workspace_bytes(long long n);
int adfp_sort_pairs(int* key, int* val, int* key_tmp, int* val_tmp, long long n, int key_bits, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Sort keys that bring a large batch of rays in INCOHERENT order (a random subset of several images' pixels) into a spatially
 * coherent one before it is rendered: key[i] = (Morton code of the ray origin's cell, 2 bits per axis) << 24 | Morton code of the
 * cell of the ray's surface point o + d * gt_depth (gt_depth <= 0 / NULL: depth 1), 8 bits per axis, both inside tsdf_bnds; val[i]
 * = i.  Sorted with adfp_sort_pairs (30 key bits) the rays of one camera that look at one 1/256 cell of the scene become
 * neighbours, and the TSDF stage's wave-wide loads and the decoders' grid gathers find their lines and pages shared again
 * (1024^3 volume, 131 072 random rays x 128 samples: 5.49 -> 4.93 ms per batch; rays are independent units, so the rendered values
 * do not depend on the order).  tsdf_bnds is a HOST array. */
int adfp_ray_sort_keys(const float* rays_o, const float* rays_d, const float* gt_depth /*or NULL*/, int n_rays, const double tsdf_bnds[3][2],
                       int* key, int* val, void* stream);
/* Is a batch in a coherent order?  Looks at up to 2048 evenly spread pairs of CONSECUTIVE rays and writes to verdict[0] how many
 * of them have surface points further apart than `far_distance` (a few TSDF voxels), and to verdict[1] the number of pairs
 * looked at.  verdict: two ints in device-visible memory (pinned host memory: the host reads it later without a sync). */
int adfp_ray_order_probe(const float* rays_o, const float* rays_d, const float* gt_depth /*or NULL*/, int n_rays, float far_distance,
                         int* verdict, void* stream);

/* ---- multi-GPU render (new functionality; the reference has no distributed code): the send / receive side of ONE all-gather ----
 * A sharded render returns several per-ray arrays (depth f64, uncertainty f64, colour 3 x f32 ... = 28 B per ray).  pack writes
 * the rank's `rows` rows of all of them interleaved into dst [rows][sum words] (the send buffer: the rank's slot of the gather
 * buffer, or a buffer padded to the largest shard); unpack reads the gathered [world][pad][sum words] buffer and writes every
 * array contiguous in ray order, rank r contributing rows_per_rank[r] <= pad rows.  Row widths in 4-byte words; at most
 * ADFP_GATHER_MAX arrays and ADFP_GATHER_MAX_RANKS ranks; src / dst / words / rows_per_rank are HOST arrays. */
#define ADFP_GATHER_MAX 8
#define ADFP_GATHER_MAX_RANKS 64
int adfp_gather_pack(int n_arrays, const void* const* src, const int* words, long long rows, void* dst, void* stream);
int adfp_gather_unpack(int n_arrays, void* const* dst, const int* words, int world, long long pad, const long long* rows_per_rank,
                       const void* gathered, void* stream);

/* Per-stage timing hook for bench.py: runs ONLY the TSDF trilerp + band-mask kernel (a10).
 * w may be NULL (that is the render path's launch: there the LOW decoder writes w = 1). */
int adfp_tsdf_stage(const adfp_scene* scene, const adfp_points* pts, unsigned char* flags,
                    int* list, float* att_u, float* w, int* counter, void* stream);

/* Per-stage timing hook for bench.py: runs ONLY one decoder kernel (kind = ADFP_DEC_LOW or ADFP_DEC_COLOR, or
 * ADFP_DEC_LOW_COLOR = the fused low + colour launch that stage color uses with f16-split images) over every point and
 * writes its output channel(s) of raw.  tile_counter: one device int the fused launch may use for its chip-wide tile tail (as it
 * does inside adfp_render_forward, where the word lives in the workspace; zeroed here before the launch), or NULL = fixed split. */
#define ADFP_DEC_LOW_COLOR 3
int adfp_decode_stage(const adfp_scene* scene, const adfp_points* pts, int kind, float* raw, float* w, int* tile_counter, void* stream);

/* ---- one sub-network alone (reference: the public modules `decoders.low_decoder / high_decoder / color_decoder / mlp`) ---- */
/* MLP.forward(p, c_grid) of src/conv_onet/models/decoder.py:177-203 for one decoder kind, no bound rule, no band logic.
 * LOW: out4 is [P,4], the value lands in channel 3 (channels 0-2 untouched); COLOR: out4 is [P,4], all four outputs of the
 * colour head (the renderer discards the fourth, decoder.py:351-352); HIGH (concat_feature: own grid + low grid): out4 is [P]. */
int adfp_decode_single(const adfp_scene* scene /*host*/, const adfp_points* pts /*host*/, int kind, float* out4, void* stream);
/* mlp_tsdf.forward of decoder.py:240-258 on explicit rows: occ [n] and the trilinear TSDF value tsdf_val [n] (adfp_sample_tsdf)
 * -> fused occupancy out4[4 i + 3] and the attention weight w[i].  scratch_u: n floats (inv_tsdf of the rows). */
int adfp_attention_rows(const adfp_scene* scene /*host*/, const float* occ, const float* tsdf_val, long long n, float* out4 /*[n,4]*/,
                        float* w /*[n]*/, float* scratch_u, void* stream);

/* ---- mesh extraction (src/utils/Mesher.py:450-486 and src/fusion.py:303-342 call skimage.measure.marching_cubes) ---- */
/* Marching cubes over a dense lattice values[nx][ny][nz] (f32, z fastest, device).  Conventions (the CPU oracle tests/mesh_ref.py
 * restates them):
 *  - a corner is inside iff v > level;
 *  - an edge carries a vertex iff both endpoints are finite and exactly one is inside; the vertex lies at
 *    t = (level - v0) / (v1 - v0) from the lower-index endpoint (f32, index space), at origin + (i + t) * spacing per axis;
 *  - point p = (i*ny + j)*nz + k owns its +x, +y and +z edges (edge key 3 p + axis): every vertex is emitted once (welded);
 *  - a cell with a non-finite corner emits nothing;
 *  - an ambiguous face (two diagonally opposite inside corners) is cut so that its inside corners are separated: the rule reads
 *    only that face, so the mesh is crack-free.  scikit-image's Lewiner decider resolves those faces differently (the vertex
 *    set, every edge crossing, is the same).  Loops are fan-triangulated from their lowest edge, so the two cells beside an
 *    ambiguous face can both draw the same diagonal between its crossings: the surface is closed and consistently oriented,
 *    but four triangles can share such an edge (not a manifold there);
 *  - order: vertices by ascending edge key, triangles by ascending cell index (the cell's lower corner), then table order.
 *    The same input gives bit-identical output; no atomics decide the order.
 * Use: adfp_mc_count (writes the totals V, F to the device array totals[2]) -> the caller reads them and allocates ->
 * adfp_mc_emit with the same values / level / workspace.  V >= 2^31 is ADFP_E_UNSUPPORTED (faces are int32); capacities below
 * the totals are ADFP_E_WORKSPACE; nothing is written past a capacity.  origin / spacing are HOST arrays; normals may be NULL
 * (else: central differences of the lattice, one-sided at the border, interpolated with t, normalised, pointing as `outward`
 * says); keys: vert_capacity edge keys (device scratch, sorted on return). */
#define ADFP_MC_MAX_TRI 5          /* triangles per case at most (tools/gen_mc_table.py asserts it) */
#define ADFP_MC_OUT_LOWER  0     /* geometric normal toward lower values (occupancy: out of the occupied region) */
#define ADFP_MC_OUT_HIGHER 1     /* toward higher values (TSDF: toward free space) */
size_t adfp_mc_workspace_bytes(int nx, int ny, int nz);
int adfp_mc_count(const float* values, int nx, int ny, int nz, float level, void* workspace, size_t workspace_bytes,
                  long long* totals, void* stream);
int adfp_mc_emit(const float* values, int nx, int ny, int nz, float level, const float origin[3], const float spacing[3], int outward,
                 const void* workspace, size_t workspace_bytes, long long n_verts, long long n_faces, float* verts, float* normals,
                 long long* keys, long long vert_capacity, int* faces, long long face_capacity, void* stream);
/* Host copy of one case's triangles (local edge ids, 3 per triangle, ADFP_MC_OUT_LOWER winding) into out[3 * ADFP_MC_MAX_TRI]
 * (host); returns the triangle count.  Corner c = (dx, dy, dz) = bits (0, 1, 2) of c; edge e = 4 * axis + the other two corner
 * bits (lower axis first). */
int adfp_mc_table(int mc_case, signed char* out);
/* The Mesher's hull mask (Mesher.py:436-439, :450): every lattice point (xs[i], ys[j], zs[k]) (f32 axes, device) for which
 * max_f(n_f . p + d_f) > 0 over the F planes [F][4] = (n, d) (f64, device) gets `fill`, in place. */
int adfp_lattice_hull_fill(float* values, const float* xs, const float* ys, const float* zs, int nx, int ny, int nz,
                           const double* planes, int n_planes, float fill, void* stream);
/* TSDFVolume.get_mesh's colours (src/fusion.py:311-319): round each index-space vertex half-to-even, read the packed colour volume
 * [nx][ny][nz] there and unpack it to r, g, b bytes (colors: [n_verts][3] uint8). */
int adfp_mesh_unpack_colors(const float* verts, long long n_verts, const float* color_vol, int nx, int ny, int nz,
                            unsigned char* colors, void* stream);

/* ---- reconstruction evaluation (src/tools/eval_recon.py, src/tools/cull_mesh.py) ----
 * Counts above 2^31 - 1025 are ADFP_E_UNSUPPORTED (indices are int32 and the radix sort's tile arithmetic is int).  Every
 * reduction is deterministic: per-workgroup partials over a grid fixed by the count, then one fixed-order pass, no float atomics,
 * so two runs on the same inputs give the same bits. */

/* Exact nearest neighbour over a reference cloud ref [n_ref][3] (f64), replacing scipy.spatial.cKDTree(ref).query
 * (eval_recon.py:33-50) and open3d's KDTreeFlann inside registration_icp (eval_recon.py:64-66).
 * adfp_nn_build fills `index` (adfp_nn_index_bytes(n_ref) bytes, the caller keeps it for the queries): the points in 30-bit
 * Morton order (their bounding box reduced on the device, adfp_sort_pairs's radix sort), grouped in leaves of 16, and an implicit
 * complete binary tree of leaf boxes (node k has children 2k, 2k+1; the leaf count is padded to a power of two with empty boxes).
 * Workspace: adfp_nn_build_workspace_bytes(n_ref), free again when the call's work has run.  n_ref = 0 builds nothing. */
size_t adfp_nn_index_bytes(long long n_ref);
size_t adfp_nn_build_workspace_bytes(long long n_ref);
int adfp_nn_build(const double* ref, long long n_ref, void* index, size_t index_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* For each query point q_i [n_query][3] (f64), transformed first by the HOST 3x4 row-major `transform` when it is not NULL
 * (x' = ((t0 x + t1 y) + t2 z) + t3, ...): dist[i] = the Euclidean distance to the nearest reference point, idx[i] = that
 * point's ORIGINAL index (any one of several at the same distance).  Squared distances are ((dx*dx + dy*dy) + dz*dz) in f64,
 * cKDTree's arithmetic.  radius: only points with d^2 < radius^2 count (INFINITY: no limit); none -> idx -1, dist +inf
 * (cKDTree's distance_upper_bound).  radius <= 0 or NaN is ADFP_E_ARG.  flags ADFP_NN_SORT_QUERIES: walk the queries in their
 * own Morton order (workspace adfp_nn_query_workspace_bytes(n_query, flags); 0 without the flag).  n_query = 0 returns 0;
 * n_ref = 0 with queries is ADFP_E_ARG. */
#define ADFP_NN_SORT_QUERIES 1
size_t adfp_nn_query_workspace_bytes(long long n_query, int flags);
int adfp_nn_query(const void* index, size_t index_bytes, long long n_ref, const double* query, long long n_query, const double transform[12],
                  double radius, int flags, void* workspace, size_t workspace_bytes, double* dist, int* idx, void* stream);
/* Workspace of the two reductions below: 8 * 17 * min(max(ceil(n / 256), 1), 1024) bytes for n elements. */
size_t adfp_recon_reduce_workspace_bytes(long long n);
/* accuracy / completion / completion_ratio (eval_recon.py:33-50): out[0] = sum of dist, out[1] = count of dist < threshold
 * (device f64 [2]); the means are those over n. */
int adfp_nn_metric_sums(const double* dist, long long n, double threshold, void* workspace, size_t workspace_bytes, double* out, void* stream);
/* The moments of one point-to-point ICP step (open3d's TransformationEstimationPointToPoint, eval_recon.py:64-66) over the
 * correspondences i with idx[i] in [0, n_tgt) (an adfp_nn_query of src under the same transform): with p = T src_i - origin,
 * q = tgt[idx[i]] - origin, out (device f64 [17]) = count, sum d^2 (d^2 as the query computes it), sum p [3], sum q [3],
 * sum p q^T [3][3] row-major.  transform [12] and origin [3] are HOST arrays. */
int adfp_icp_moments(const double* src, long long n_src, const double transform[12], const double origin[3], const double* tgt, long long n_tgt,
                     const int* idx, void* workspace, size_t workspace_bytes, double* out, void* stream);
/* trimesh.sample.sample_surface(mesh, count) (eval_recon.py:115-118) on caller-drawn uniforms u_face [count], u_bary [count][2]
 * (f64): face areas |cross(v1 - v0, v2 - v0)| / 2, their inclusive scan cum (fixed order; where the parallel scan's rounding
 * would let cum step down by an ulp, it is held at the larger value before it, so cum never decreases), face = first f with
 * cum[f] >= u_face * cum[F-1] (numpy searchsorted, side='left'), (a, b) = u_bary folded (a + b > 1: both minus 1, then absolute
 * values), point = (a (v1 - v0) + b (v2 - v0)) + v0.  Out: points [count][3] f64, face_index [count] int32.  A face with an
 * index outside [0, n_verts) has area 0.  Workspace: adfp_sample_surface_workspace_bytes(n_faces) = 8 n_faces rounded up to
 * 256, plus 8 (2 ceil(n_faces / 2048) + 1).  count = 0 returns 0; no faces with draws is ADFP_E_ARG. */
size_t adfp_sample_surface_workspace_bytes(long long n_faces);
int adfp_sample_surface(const double* verts, long long n_verts, const int* faces, long long n_faces, const double* u_face, const double* u_bary,
                        long long count, void* workspace, size_t workspace_bytes, double* points, int* face_index, void* stream);
/* cull_mesh.py:49-71 over every pose in one launch (no workspace): seen[i] = 1 iff some pose sees vertex i.  w2c [n_poses][12]
 * (f32, device) = the top three rows of inv(c2w) (the caller inverts in f64 and rounds to f32, as np.linalg.inv of the f32 pose
 * does); with p the f32 rounding of verts[i] (f64): cam = w2c [p, 1], cam.x *= -1, uv = K cam, z = uv.z + 1e-5, uv /= z,
 * seen iff 0 <= -z && 0 < u < W && 0 < v < H, all in f32. */
int adfp_cull_vertices(const double* verts, long long n_verts, const float* w2c, long long n_poses, float fx, float fy, float cx, float cy,
                       int W, int H, unsigned char* seen, void* stream);
/* cull_mesh.py:72-74: keep[f] = 0 iff all three vertices of face f are unseen (an index outside [0, n_verts) counts as unseen). */
int adfp_cull_faces(const unsigned char* seen, long long n_verts, const int* faces, long long n_faces, unsigned char* keep, void* stream);

/* ---- mesh depth rendering (eval_recon.py:139-219, calc_2d_metric) ----
 * Triangle BVH.  adfp_tri_bvh_build fills `bvh` (adfp_tri_bvh_bytes(n_faces, leaf) bytes, kept by the caller for the renders):
 * the faces in 30-bit Morton order of their centroids ((v0 + v1) + v2) / 3 (the NN index's box, code and sort passes), in leaves
 * of `leaf` triangles (4, 8 or 16; ADFP_TRI_LEAF_DEFAULT) that hold each triangle's nine f64 vertex coordinates and its original
 * face index, and an implicit complete binary tree of leaf boxes (node k has children 2k, 2k+1; the leaf count is padded to a power
 * of two with inverted boxes).  A face with an index outside [0, n_verts) is never hit.  Workspace:
 * adfp_tri_bvh_build_workspace_bytes(n_faces) = 24 n_faces rounded up to 256 plus adfp_nn_build_workspace_bytes(n_faces).
 * n_faces = 0 builds nothing.  bvh bytes: 72 n_faces and 4 n_faces, each rounded up to 256, plus 96 P (P = leaves rounded up to a
 * power of two). */
#define ADFP_TRI_LEAF_DEFAULT 4
size_t adfp_tri_bvh_bytes(long long n_faces, int leaf);
size_t adfp_tri_bvh_build_workspace_bytes(long long n_faces);
int adfp_tri_bvh_build(const double* verts, long long n_verts, const int* faces, long long n_faces, int leaf, void* bvh, size_t bvh_bytes,
                       void* workspace, size_t workspace_bytes, void* stream);
/* Depth images of n_views views in one launch: depth [n_views][H][W] (f32, device).  c2w [n_views][12] (f64, device) = the top three
 * rows of each camera-to-world matrix [R | o], R a rotation; near [n_views] (f64, device) per view, `far` shared (host).
 *   Camera: OpenCV axes (x right, y down, z forward), the extrinsic inv(c2w) of open3d's PinholeCameraParameters.  Pixel (row i,
 *     col j) has d = ((j - cx) / fx, (i - cy) / fy, 1) in camera space, in f64 in that order; the world ray is o + t R d, so t is
 *     camera z.
 *   Intersection: Woop, Benthin & Wald (2013), watertight, in f64, the axis permutation fixed to z and the shear Sx = -dx,
 *     Sy = -dy, Sz = 1.  Each vertex v goes to camera space first: e = v - o (per component), cam_c = ((R0c e0 + R1c e1) + R2c e2).
 *     Then Ax' = Ax - dx Az, Ay' = Ay - dy Az (the same for B, C); U = Cx' By' - Cy' Bx', V = Ax' Cy' - Ay' Cx',
 *     W = Bx' Ay' - By' Ax'.  A miss when U, V, W have mixed signs or det = (U + V) + W is 0, else z = ((U Az + V Bz) + W Cz) / det.
 *     Edges count as inside (a ray through a shared edge or vertex hits at least one of its triangles); back faces count.
 *   Depth: the least z over all hits with near <= z <= far, rounded to f32; 0 where there is none.  Clipping is per pixel (GL
 *     clipping followed by a z-buffer).  The result is a minimum over a set: independent of the traversal order, equal to a brute
 *     force over all faces bit for bit (tests/depth_ref.py), two runs give the same bits.
 *   Pruning is conservative: every box tested is first grown by 2^-24 (max |coordinate| of the mesh's box + max |o|), a margin
 *     far above the rounding of both the slab test and the triangle test, so boxes of zero thickness keep a width; an axis along
 *     which R d is 0 (|R d| < 1e-200) is a containment test instead of a slab, so no 0 x inf arises.  The walk is the stackless
 *     trail-bit walk that k_nn_query runs (bvh_walk, csrc/adfp_recon.h): the child with the smaller entry t first, a box pruned when its entry t exceeds the best z or its
 *     exit t lies below near.
 * n_faces = 0 writes zeros (bvh, c2w and near may be NULL); n_views = 0 does nothing.  far must be positive and finite, fx, fy
 * nonzero; H, W in [1, 32768]. */
int adfp_render_depth(const void* bvh, size_t bvh_bytes, long long n_faces, int leaf, const double* c2w, const double* near, double far,
                      long long n_views, int H, int W, double fx, double fy, double cx, double cy, float* depth, void* stream);
/* The same render with back- or front-face culling (pyrender's GL_CULL_FACE, evaluate_scannet.py:120-136).  cull = ADFP_CULL_NONE
 * is adfp_render_depth bit for bit (the same kernel).  Facing is the sign of the watertight test's det = (U + V) + W: in real
 * arithmetic det = -(n . R d) with n = (v1 - v0) x (v2 - v0) (the shear has determinant 1), so det > 0 is a FRONT face, one whose
 * normal points toward the camera (GL's counter-clockwise front face, seen from the camera), and det < 0 a BACK face.
 * ADFP_CULL_BACK keeps only hits with det > 0, ADFP_CULL_FRONT only hits with det < 0.  In the culled modes a view whose c2w holds
 * a non-finite entry is all zeros.  Another cull value is ADFP_E_ARG; the other arguments and errors are adfp_render_depth's. */
#define ADFP_CULL_NONE  0
#define ADFP_CULL_BACK  1
#define ADFP_CULL_FRONT 2
int adfp_render_depth_cull(const void* bvh, size_t bvh_bytes, long long n_faces, int leaf, const double* c2w, const double* near,
                           double far, long long n_views, int H, int W, double fx, double fy, double cx, double cy, int cull,
                           float* depth, void* stream);
/* ---- mesh views: which triangle a pixel sees, where on it, and what it looks like ----
 * The hit render: adfp_render_depth_cull's arguments, argument checks, errors, launch geometry and walk, with three outputs (device),
 * each of which may be NULL but not all three (ADFP_E_ARG):
 *   depth [n_views][H][W] f32     adfp_render_depth_cull's image for the same arguments bit for bit (the culled modes' all-zero view
 *                                 for a pose with a non-finite entry included).
 *   face  [n_views][H][W] int32   the ORIGINAL index (row of the faces given to adfp_tri_bvh_build) of the nearest hit; -1 exactly
 *                                 where no triangle passes the test above with near <= z <= far (a hit at z = 0 with near = 0 has
 *                                 depth 0 and a face).  The nearest hit is the one of least f64 z, z as stated above; among hits
 *                                 whose z are equal as doubles the smallest original index wins.  The walk's bound is closed (a
 *                                 triangle at exactly the best z is tested, a box entered at exactly the best z is walked), so every
 *                                 tied triangle is visited: face is a function of the set of hits, not of the traversal, the leaf
 *                                 size or the run, and equals a brute force over all faces (tests/hits_ref.py).
 *   bary  [n_views][H][W][2] f32  (V / det, W / det) of the winning triangle, the weights of its v1 and v2 (U belongs to v0:
 *                                 z = ((U Az + V Bz) + W Cz) / det), each divided in f64 and then rounded to f32; (0, 0) where
 *                                 face is -1.
 * n_faces = 0 writes 0 / -1 / (0, 0); n_views = 0 does nothing. */
int adfp_render_hits(const void* bvh, size_t bvh_bytes, long long n_faces, int leaf, const double* c2w, const double* near, double far,
                     long long n_views, int H, int W, double fx, double fy, double cx, double cy, int cull, float* depth, int* face,
                     float* bary, void* stream);
/* Area-weighted vertex normals (open3d's TriangleMesh.compute_vertex_normals as we read it -- unnormalised triangle normals summed
 * per vertex, then normalised; unpinned: there is no open3d to compare against), deterministic, no float atomics.  verts
 * [n_verts][3] f64, faces [n_faces][3] int32, normals [n_verts][3] f64 (device).  Per face, in f64, every difference and product
 * rounded on its own: e1 = v1 - v0, e2 = v2 - v0, n_f = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x); a face with an
 * index outside [0, n_verts) is skipped.  Per vertex: s = 0, then s += n_f (per component) over its incident face corners in
 * ascending face index (a face that names the vertex twice adds twice); len = sqrt((sx sx + sy sy) + sz sz); normal = s / len
 * (per component), or (0, 0, 0) when len is 0 or not finite (an unreferenced vertex among them).  Workspace:
 * adfp_vertex_normals_workspace_bytes(n_faces) = 24 n_faces and four times 12 n_faces, each rounded up to 256, plus
 * adfp_sort_workspace_bytes(3 n_faces) rounded up to 256 (0 for n_faces <= 0 or beyond the limit).  n_verts = 0 does nothing;
 * n_faces = 0 writes zeros (faces and workspace may be NULL).  n_verts or 3 n_faces above 2^31 - 1025 is ADFP_E_UNSUPPORTED. */
size_t adfp_vertex_normals_workspace_bytes(long long n_faces);
int adfp_vertex_normals(const double* verts, long long n_verts, const int* faces, long long n_faces, void* workspace,
                        size_t workspace_bytes, double* normals, void* stream);
/* The shading pass over adfp_render_hits's face and bary images (device; a caller may also make them): one lane per pixel, every
 * operation below in f64 in the order written, no contraction.  verts, faces: the mesh given to adfp_tri_bvh_build; c2w
 * [n_views][12] and fx, fy, cx, cy: the render's.  vertex_normals [n_verts][3] f64 (device) or NULL = flat shading;
 * vertex_colors [n_verts][3] u8 (device) or NULL = the uniform `albedo` (HOST, three floats, widened to f64); `background` (HOST,
 * three bytes).  Outputs (device), each may be NULL: normal [n_views][H][W][3] f32, rgb [n_views][H][W][3] u8.
 *   No hit: face < 0, face >= n_faces, or a face with a vertex index outside [0, n_verts) (the last two cannot come from
 *     adfp_render_hits).  normal = (0, 0, 0), rgb = background.
 *   Weights: b1, b2 = the f32 bary values widened; b0 = (1 - b1) - b2.
 *   Geometric normal: g = (v1 - v0) x (v2 - v0) as in adfp_vertex_normals.
 *   Shading normal: n = g when vertex_normals is NULL, else s_c = (b0 n0_c + b1 n1_c) + b2 n2_c with n0, n1, n2 the normals of
 *     v0, v1, v2, and n = s unless all three components of s equal 0, then n = g.
 *   Camera space, in the vertex transform's order: m_c = (R0c n_0 + R1c n_1) + R2c n_2 (R transposed).  len = sqrt((m_0 m_0 +
 *     m_1 m_1) + m_2 m_2); m = m / len per component, or (0, 0, 0) when len is 0 or not finite.  With d = (dx, dy, 1) the pixel's
 *     direction as in the render, t = (m_0 dx + m_1 dy) + m_2; when t > 0 both m and t are negated: every normal faces the camera.
 *   normal = m rounded to f32.
 *   Intensity: I = ambient + (1 - ambient) * (-t / sqrt((dx dx + dy dy) + 1)): a light at the camera.
 *   Base colour: ((b0 c0 + b1 c1) + b2 c2) / 255 per channel with c0, c1, c2 the bytes of v0, v1, v2 widened, or the albedo.
 *   rgb, by mode: ADFP_SHADE_COLOR x = base; ADFP_SHADE_SHADED x = base * I; ADFP_SHADE_NORMAL x = ((m_0 + 1) / 2,
 *     (-m_1 + 1) / 2, (-m_2 + 1) / 2) (the OpenGL-axes normal map).  byte = floor(y * 255 + 0.5) with y = x when x > 0 else 0
 *     (NaN goes to 0), then y = y when y < 1 else 1.
 * A byte whose y * 255 lies within rounding of a half-integer may differ by one from another correctly rounded evaluation only if
 * sqrt or division were not correctly rounded; they are (tests/test_gpu_mesh_shade.py compares against numpy).
 * ADFP_E_ARG: a NULL face, bary, c2w or background, NULL albedo without vertex_colors, NULL verts or faces with n_faces > 0, a
 * negative count, H or W < 1, a mode other than the three, ambient outside [0, 1] or NaN, fx or fy zero or an intrinsic not finite.
 * ADFP_E_UNSUPPORTED: H or W above 32768, a count above 2^31 - 1025, more than 2^38 pixels.  n_views = 0, or both outputs NULL,
 * does nothing. */
#define ADFP_SHADE_COLOR  0
#define ADFP_SHADE_SHADED 1
#define ADFP_SHADE_NORMAL 2
int adfp_shade_hits(const int* face, const float* bary, long long n_views, int H, int W, const double* verts, long long n_verts,
                    const int* faces, long long n_faces, const double* c2w, double fx, double fy, double cx, double cy,
                    const double* vertex_normals, const unsigned char* vertex_colors, const float albedo[3] /*host*/, double ambient,
                    const unsigned char background[3] /*host*/, int mode, float* normal, unsigned char* rgb, void* stream);
/* 3D line segments drawn over such views with the mesh in the way (a trajectory, a camera frustum): rgb [n_views][H][W][3] u8
 * (device) is painted in place, depth [n_views][H][W] f32 (device: adfp_render_hits's, or NULL = nothing occludes), seg
 * [n_views][H][W] int32 (device, or NULL) receives per pixel the index of the segment drawn there.  c2w [n_views][12] and fx, fy, cx,
 * cy are the render's; segments [n_seg][2][3] f64 world endpoints and colors [n_seg][3] u8 (device) are ONE list shared by all
 * views; ranges [n_views][n_ranges][2] int64 (device; NULL = every view draws [0, n_seg)) says which part of it each view draws.
 * Everything below is f64, one operation at a time in the order written, no contraction; the camera, axes and pixel centres are
 * adfp_render_depth's: pixel (row i, col j) has its centre at the screen point (j, i).  rgb and seg are a function of the arguments
 * alone: the same bytes every run, equal to a brute force over all pixels and listed segments (tests/segments_ref.py).
 *   View: a view whose 12 pose entries are not all finite is left untouched; its seg is -1.
 *   Listed segments: view v draws segment k iff one of its ranges [b, e) holds k, b <= k < e.  Ranges are clamped to [0, n_seg); an
 *     empty or inverted range holds nothing; a segment held by two ranges counts once.  n_listed (host) must be at least the largest
 *     sum over a view's ranges of their clamped lengths (a segment held twice counted twice): the listed segments are laid out
 *     range after range and what lies beyond n_listed is not drawn.  Without ranges n_listed is not read (it is n_seg).
 *   Camera space per endpoint P, as the depth render's vertices: e = P - o, cam_c = ((R0c e0 + R1c e1) + R2c e2).  A segment with a
 *     non-finite endpoint coordinate draws nothing.
 *   Near clip, endpoints A and B: both Az < near_clip and Bz < near_clip: nothing.  Else if Az < near_clip: t = (near_clip - Az) /
 *     (Bz - Az) and A becomes (Ax + t (Bx - Ax), Ay + t (By - Ay), near_clip); else if Bz < near_clip the same with A and B
 *     exchanged.
 *   Screen per endpoint: u = fx (x / z) + cx, v = fy (y / z) + cy, w = 1 / z.  A non-finite u, v or w: nothing.
 *   Coverage of pixel (i, j): a = (u1 - u0, v1 - v0), dw = w1 - w0, L = ax ax + ay ay; p = (j - u0, i - v0); s = 0 when L is 0, else
 *     (px ax + py ay) / L; s = s when s > 0 else 0 (NaN goes to 0), then s = 1 when s > 1; q = (px - s ax, py - s ay).  The pixel is
 *     covered iff qx qx + qy qy <= half_width half_width: round caps, no antialiasing, no square root.
 *   Depth of the line at the pixel, perspective-correct: z = 1 / (w0 + s dw).
 *   Winner: among the listed segments that cover the pixel the one of least z; among equal z the smallest index k.  The winner is
 *     the minimum over a set: it does not depend on tiles, on the order of the ranges or on the run.  seg = its k, or -1.
 *   Visibility of the winner, D the pixel's depth value widened: visible when depth is NULL, or D is 0 (nothing hit), or
 *     z <= D (1 + bias_rel) + bias_abs.  Visibility is monotone in z: if any covering segment is visible, the winner is.
 *   Paint: visible: the three bytes become colors[k].  Hidden with hidden_alpha > 0: per channel byte = floor((hidden_alpha c +
 *     (1 - hidden_alpha) p) + 0.5), c the segment's byte and p the old one, widened.  Hidden with hidden_alpha 0: unchanged.
 * Two launches per 32768 views: one lane per (view, listed slot) projects it into a 64-byte record of the workspace
 * (adfp_draw_segments_workspace_bytes(n_views, n_listed) = 64 n_views n_listed rounded up to 256; 0 for a count that is not positive
 * or beyond the limits); one workgroup per 16 x 16 pixel tile and view then reads the view's records 256 at a time, drops those
 * whose box misses the tile grown by half_width + 1 pixels and tests the rest per pixel.  No atomics; one write per pixel.
 * ADFP_E_ARG, before any launch: NULL rgb or c2w; NULL segments or colors with n_seg > 0; a negative count; H or W < 1; fx or fy
 * zero or an intrinsic not finite; half_width outside (0, 64]; near_clip not positive and finite; a negative or non-finite bias;
 * hidden_alpha outside [0, 1] or NaN; n_ranges outside [1, 8] with ranges; a NULL or too small workspace when something is listed.
 * ADFP_E_UNSUPPORTED: H or W above 32768, a count above 2^31 - 1025, n_views n_listed above 2^34.  n_views = 0 does nothing; n_seg = 0
 * or n_listed = 0 leaves rgb as it is and writes -1 to seg (the workspace may be NULL). */
size_t adfp_draw_segments_workspace_bytes(long long n_views, long long n_listed);
int adfp_draw_segments(unsigned char* rgb, const float* depth, int* seg, long long n_views, int H, int W, const double* c2w,
                       double fx, double fy, double cx, double cy, const double* segments, const unsigned char* colors,
                       long long n_seg, const long long* ranges, int n_ranges, long long n_listed, double half_width,
                       double near_clip, double bias_rel, double bias_abs, double hidden_alpha, void* workspace,
                       size_t workspace_bytes, void* stream);
/* check_proj (eval_recon.py:70-96) for a batch of poses: any[p] (int32, device) = 1 iff pose p projects some point into the
 * image, else 0.  w2c [n_poses][12] (f32, device) = the top three rows of inv(c2w'), c2w' = c2w with columns 1 and 2 negated,
 * inverted in f64 and rounded to f32 by the caller; the per-point test is adfp_cull_vertices's.  n_poses = 0 does nothing;
 * no points gives all zeros. */
int adfp_views_in_sight(const double* points, long long n_points, const float* w2c, long long n_poses, float fx, float fy, float cx, float cy,
                        int W, int H, int* any, void* stream);
/* Occlusion-aware visibility of points from a batch of poses in one launch (no workspace): seen[i] (device) = 1 iff some pose k
 * both (a) has point i in its frustum and (b) sees it unoccluded by the mesh of `bvh` (adfp_tri_bvh_build's, with its n_faces and
 * leaf), else 0.
 *   (a) is adfp_cull_vertices's test bit for bit: w2c [n_poses][12] (f32, device) are its rows, the point (f64) is rounded to f32.
 *   (b) is a shadow ray in adfp_render_depth's arithmetic: c2w [n_poses][12] (f64, device) = the top three rows [R | o] of the same
 *     pose in OpenCV axes.  The point p goes to camera space as a mesh vertex does, e = p - o, cam_c = ((R0c e0 + R1c e1) + R2c e2),
 *     and z_p = cam_z.  The pair is not visible when z_p <= 0 or is not finite, when d = (cam_x / z_p, cam_y / z_p, 1) is not
 *     finite, or when the pose's c2w row holds a non-finite entry.  Else the triangle test is the one above verbatim with that d
 *     (the shear, U, V, W; mixed signs or det = 0 miss; z = ((U Az + V Bz) + W Cz) / det; edges inside, back faces count), and the
 *     point is occluded iff some triangle is hit with near <= z && z < z_p - eps.  eps keeps a surface point from being occluded
 *     by the face it lies on.  The decision is existence over a set of hits: independent of the traversal order, equal to a brute
 *     force over all faces (tests/visible_ref.py), two runs give the same bytes.
 *   The walk is the renderer's with the bound fixed at z_p - eps: boxes padded as there, a box pruned when its entry t is at or
 *     beyond the bound or its exit t lies below near, left at the first qualifying hit.  Only pairs that pass (a) are walked, and
 *     a point that some pose has seen is not tested against the poses after it.
 * n_faces = 0 returns exactly what adfp_cull_vertices returns (bvh and c2w may be NULL).  n_points = 0 returns 0; n_poses = 0
 * writes zeros.  ADFP_E_ARG: a NULL pointer, a negative count, a leaf other than 4, 8, 16, eps or near negative or not finite,
 * fx or fy zero. */
int adfp_points_visible(const void* bvh, size_t bvh_bytes, long long n_faces, int leaf, const double* points, long long n_points,
                        const float* w2c, const double* c2w, long long n_poses, float fx, float fy, float cx, float cy, int W, int H,
                        double near, double eps, unsigned char* seen, void* stream);
/* Per view p: out[p] (f64, device) = sum over n_pixels of (double)|a - b|, the f32 difference widened, for a, b [n_views][n_pixels]
 * (f32, device); per-workgroup partials over min(max(ceil(n_pixels / 256), 1), 1024) workgroups, then one fixed-order pass.
 * Workspace: adfp_depth_l1_workspace_bytes = 8 n_views times that workgroup count.  n_views = 0 does nothing. */
size_t adfp_depth_l1_workspace_bytes(long long n_views, long long n_pixels);
int adfp_depth_l1_sums(const float* a, const float* b, long long n_views, long long n_pixels, void* workspace, size_t workspace_bytes,
                       double* out, void* stream);

/* ---- ScanNet mesh evaluation (src/tools/evaluate_scannet.py: refuse, evaluate) ----
 * refuse() renders the predicted mesh from every 10th pose and fuses the depths into open3d's ScalableTSDFVolume.  open3d is not
 * a dependency; the three entries below are our reading of its legacy integration (unpinned: no open3d to compare against), over a
 * DENSE box of whole units instead of a hash map of them.  A unit is ADFP_UNIT_VOXELS^3 voxels; unit (a, b, c) covers world voxel
 * indices 16 a .. 16 a + 15 (per axis), and world voxel k has its centre at (k + 0.5) voxel.  A box is unit_lo[3] (HOST, world
 * unit indices of its first unit) and unit_dim[3] (HOST, units per axis, each >= 1); its units are numbered (a dim1 + b) dim2 + c
 * (relative indices), its voxels form the lattice [16 dim0][16 dim1][16 dim2], z fastest.  A box of more than 2^31 - 1 units is
 * ADFP_E_UNSUPPORTED. */
#define ADFP_UNIT_VOXELS 16
/* Unit touch marks (ScalableTSDFVolume::Integrate's allocation): for view p of n_views and each pixel (row v, col u) with
 * u % stride == 0 and v % stride == 0 of depth [n_views][H][W] (f32, device) whose d satisfies 0 < d <= depth_trunc (f32):
 * x = ((u - cx) d) / fx, y = ((v - cy) d) / fy, and the point P = ((m0 x + m1 y) + m2 d) + m3 per row of c2w [n_views][12] (f64,
 * device; the camera pose that back-projects, open3d's extrinsic.inverse()), all in f64.  Every unit from floor((P - sdf_trunc) /
 * unit_length) to floor((P + sdf_trunc) / unit_length), per axis, gets touched[p][unit] = 1 (u8, device, [n_views][units of the
 * box]; zeroed by the call first; plain stores of 1, no atomics).  A point with a non-finite bound touches nothing (nothing
 * non-finite is converted to an integer).  A point whose range reaches outside the box marks the part inside and adds 1 to
 * *outside (one device int; never zeroed by the call: the caller zeroes it and checks it is 0).  n_views = 0 does nothing.
 * Errors: ADFP_E_ARG for a null pointer, n_views < 0, H or W < 1, stride < 1, fx or fy 0 or non-finite, cx or cy non-finite,
 * sdf_trunc < 0 or non-finite, unit_length <= 0 or non-finite, depth_trunc <= 0, unit_dim < 1; ADFP_E_UNSUPPORTED for H or
 * W > 32768 and the box above. */
int adfp_refuse_touch(const float* depth, long long n_views, int H, int W, const double* c2w, double fx, double fy, double cx, double cy,
                      int stride, float depth_trunc, double sdf_trunc, double unit_length, const int unit_lo[3], const int unit_dim[3],
                      unsigned char* touched, int* outside, void* stream);
/* Unit-gated integration of a chunk of views (IntegrateWithDepthToCameraDistanceMultiplier as we read it), in place on tsdf and
 * weight (f32, device, the box's lattice).  units [n_units] (int32, device): the unit ids to visit (ids outside the box are
 * skipped); normally those that some view of the chunk touched.  For every voxel of a listed unit and for each view k of
 * [0, n_views) IN ORDER with touched[k][unit] != 0 (so that chunking never changes a bit), with (x, y, z) the voxel centre
 * ((k_c + 0.5) voxel in f64, rounded to f32) and w2c [n_views][12] (f32, device; inv(pose) in f64 rounded to f32), all in f32:
 *   cam = ((r0 x + r1 y) + r2 z) + t per row; cam.z <= 0 (or NaN) skips the view;
 *   u_f = ((cam.x fx) / cam.z + cx) + 0.5f, v_f likewise; the voxel is used only if 0.0001 <= u_f < W - 0.0001 and
 *   0.0001 <= v_f < H - 0.0001 (W - 0.0001f in f32); u = (int)u_f, v = (int)v_f;
 *   d = depth[k][v][u]; a d outside (0, depth_trunc] is no observation;
 *   sdf = (d - cam.z) * sqrtf((du du + dv dv) + 1), du = (u - cx) / fx, dv = (v - cy) / fy (correctly rounded sqrt and divisions);
 *   if sdf > -sdf_trunc: t = fminf(1, sdf * (1 / sdf_trunc)), tsdf = (tsdf w + t) / (w + 1), w = w + 1.
 * Voxels of units not listed keep their values.  n_units = 0 or n_views = 0 does nothing.  Errors: ADFP_E_ARG for a null pointer,
 * n_units or n_views < 0, H or W < 1, voxel or sdf_trunc <= 0 or non-finite, depth_trunc <= 0, fx or fy 0 or non-finite, cx or cy
 * non-finite, unit_dim < 1; ADFP_E_UNSUPPORTED for n_units above the box's unit count, n_views > 65536, H or W > 32768 and the box
 * above. */
int adfp_refuse_integrate(float* tsdf, float* weight, const int unit_lo[3], const int unit_dim[3], double voxel, const int* units,
                          long long n_units, const float* depth, const float* w2c, const unsigned char* touched, long long n_views, int H,
                          int W, float fx, float fy, float cx, float cy, float sdf_trunc, float depth_trunc, void* stream);
/* open3d's PointCloud::voxel_down_sample as we read it, over points [n][3] (f64, device) whose bounds the caller passes
 * (min_bound, max_bound: HOST f64 [3], the exact per-axis minimum and maximum of the points): vmin = min_bound - voxel_size * 0.5,
 * cells per axis N_c = floor((max_bound_c - vmin_c) / voxel_size) + 1 (more than 2^21 is ADFP_E_UNSUPPORTED), a point's cell
 * i_c = floor((p_c - vmin_c) / voxel_size), its key (i_0 N_1 + i_1) N_2 + i_2.  The points are sorted stably by key with
 * adfp_sort_pairs, in passes of 31 key bits from the lowest when the key is wider.  out [n][3] (f64, device, capacity n) gets one
 * point per occupied cell in ascending key order: the f64 sum of its points, in input order, over their count (each component
 * divided); counts [n] (int32) the counts; total (one device long long) the number of cells.  Deterministic: no atomics decide
 * anything.  Workspace: adfp_voxel_down_sample_workspace_bytes(n) = 8 n + 5 x 4 n + 4 T + 8 T + adfp_sort_workspace_bytes(n),
 * each rounded up to 256, T = ceil(n / 1024); 0 for n <= 0.  n = 0 writes total = 0.  Errors: ADFP_E_ARG for a null pointer, n < 0,
 * voxel_size <= 0 or non-finite, non-finite bounds or min_bound > max_bound; ADFP_E_UNSUPPORTED for n > 2^31 - 1025;
 * ADFP_E_WORKSPACE. */
size_t adfp_voxel_down_sample_workspace_bytes(long long n);
int adfp_voxel_down_sample(const double* points, long long n, double voxel_size, const double min_bound[3], const double max_bound[3],
                           void* workspace, size_t workspace_bytes, double* out, int* counts, long long* total, void* stream);
/* ---- The Mapper's overlap keyframe selection (src/Mapper.py:160-222, Mapper.keyframe_selection_overlap) ----------------------
 * counts[k] (int32, device, [K]) = how many of the current frame's n * N_samples sample points keyframe k sees, in ONE launch.
 * Sample points: idx [n] (int64, device) are the caller's one torch.randint draw over H W (pixel idx[t] = row idx / W, column
 * idx % W of the [H,W] f32 depth_img); ray t is adfp_rays_from_uv's through that pixel under c2w (device, row-major [4,4] f32, with
 * fx .. cy rounded to f32); sample s of N_samples has t_s = torch.linspace(0, 1, N_samples)[s] (torch's CPU rule: step =
 * 1 / (N_samples - 1) in f32, t_s = fma(step, s, 0) for s < N_samples / 2, else fma(-step, N_samples - 1 - s, 1)); with d the
 * pixel's depth, near = d 0.8, far = d + 0.5, z = near (1 - t_s) + far t_s and point = o + d_ray z, every other product and sum
 * rounded on its own in f32.  Point q = t N_samples + s goes to pts_out [q][3] (f32, device) when pts_out is not NULL.
 * Inside test per keyframe: w2c = inverse of poses[k] (row-major [4,4] f32, device; inverted in f64 and rounded to f32);
 * cam = ((w0 x + w1 y) + w2 z) + w3 per row of w2c in f32; X = -cam.x; in f64: Z = cam.z + 1e-5, u = (fx X + cx cam.z) / Z,
 * v = (fy cam.y + cy cam.z) / Z, both rounded to f32; inside = edge < u < W - edge and edge < v < H - edge (in f32) and Z < 0.
 * A drawn index outside [0, H W) gives a NaN point (inside nowhere); a singular pose sees nothing.  Deterministic (no atomics).
 * K = 0 launches nothing (pts_out is not written).  Errors: ADFP_E_ARG for K < 0, n <= 0, N_samples < 1, H or W < 1, a null idx,
 * depth_img, c2w or counts, null poses with K > 0, fx or fy 0 or non-finite, cx or cy non-finite; ADFP_E_UNSUPPORTED for
 * n N_samples above 2^31 - 4097. */
int adfp_keyframe_overlap(const long long* idx, int n, const float* depth_img, int H, int W, const float* c2w, int N_samples,
                          const float* poses, int K, double fx, double fy, double cx, double cy, int edge, int* counts, float* pts_out,
                          void* stream);

/* ---- mesh clean-up (src/utils/Mesher.py:58-217 point masks, :492-513 the trimesh culling, Trimesh(process=True)'s vertex merge) ----
 * Everything between marching cubes and the file, on the device.  Meshes: verts [V][3] f32, faces [F][3] int32.  V above
 * 2^31 - 1025 or 3 F above 2^31 - 1025 is ADFP_E_UNSUPPORTED (the half-edges are sorted with adfp_sort_pairs); a null pointer or a
 * negative count ADFP_E_ARG; a short workspace ADFP_E_WORKSPACE.  A face with an index outside [0, V) is never dereferenced: it
 * gets no label, is never kept, and maps to -1 in a merge.  No atomics decide a result; the same input gives the same bits. */

/* The Mesher's *seen* mask over every pose in one launch (no workspace): seen[i] = 1 iff some pose p sees vertex i.  w2c
 * [n_poses][12] (f32, device) = the top three rows of inv(c2w) as np.linalg.inv of the f32 pose gives them.  Mesher._project in
 * f32, each product and sum rounded on its own: cam = ((w0 x + w1 y) + w2 z) + w3 per row, X = -cam.x, Z = cam.z, zz = Z + 1e-8,
 * u = (fx X + cx Z) / zz, v = (fy cam.y + cy Z) / zz; frustum: zz < 0 && 0 < u < W && 0 < v < H.  rule:
 *   ADFP_SEEN_FRUSTUM     the frustum only (get_mask_use_all_frames);
 *   ADFP_SEEN_MAX_DEPTH   and -Z < depth_max[p] (depth_test = False; depth_max [n_poses] f32: the caller's 1.1 * max(depth[p]));
 *   ADFP_SEEN_DEPTH_TEST  and d - 2.4 < -Z < d + 2.4 with d = F.grid_sample(depth[p], bilinear, zeros, align_corners=True) at the
 *                         grid the Mesher forms: g = (u * (1 / (W - 1))) * 2 - 1, ix = ((g + 1) / 2) * (W - 1) (likewise v, H), corner
 *                         weights (x1 - ix)(y1 - iy), (ix - x0)(y1 - iy), (x1 - ix)(iy - y0), (ix - x0)(iy - y0), products summed in
 *                         that order, corners outside the image skipped; depth [n_poses][H][W] f32.  H or W < 2: ADFP_E_UNSUPPORTED.
 * The forecast / unseen masks are not computed.  Another rule, a rule without its depth array, H or W < 1: ADFP_E_ARG; H or
 * W > 32768, n_poses > (2^31 - 1025) / 12: ADFP_E_UNSUPPORTED.  n_poses = 0 writes zeros. */
#define ADFP_SEEN_FRUSTUM    0
#define ADFP_SEEN_MAX_DEPTH  1
#define ADFP_SEEN_DEPTH_TEST 2
int adfp_mesh_seen_mask(const float* verts, long long n_verts, const float* w2c, long long n_poses, int rule, const float* depth,
                        const float* depth_max, float fx, float fy, float cx, float cy, int W, int H, unsigned char* seen, void* stream);

/* Face components as trimesh.split forms them: two faces are joined only through an edge {a, b} that EXACTLY two half-edges use
 * (a face (a, a, c) uses {a, c} twice and joins nothing).  A face takes part iff keep is NULL or keep[f] != 0, and its indices
 * lie in [0, n_verts).  _begin orders the 3 F half-edges by (min, max) with two stable sorts and writes mate [3 F] (int32: the
 * face across half-edge 3 f + c, or -1) and the start labels[f] = f (-1 for a face that takes no part).  _rounds runs `rounds`
 * rounds of: every mate pair with different roots hooks the larger root under the smaller (atomicMin), then every face points at
 * its root; *changed (one device int) = 1 iff the LAST of them hooked anything.  The caller repeats _rounds until it reads 0;
 * then labels[f] = the smallest face index of f's component.  Labels only descend, so every walk ends, and 2 log2(F) + 2 rounds
 * are the worst case (csrc/adfp_meshclean.h).  Workspace of _begin: 6 x 12 F bytes, each rounded up to 256, plus
 * adfp_sort_workspace_bytes(3 F); free after the call.  n_faces = 0 does nothing (changed = 0). */
size_t adfp_mesh_face_labels_workspace_bytes(long long n_faces);
int adfp_mesh_face_labels_begin(const int* faces, long long n_faces, long long n_verts, const unsigned char* keep /*or NULL*/, int* mate,
                                int* labels, void* workspace, size_t workspace_bytes, void* stream);
int adfp_mesh_face_labels_rounds(const int* mate, int* labels, long long n_faces, int rounds, int* changed, void* stream);

/* The keep rule of Mesher.py:497-510 on final labels: area[f] = 0.5 |cross(v1 - v0, v2 - v0)| in f64 from the f32 vertices, as
 * numpy forms it (cross = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), no FMA, sqrt((x x + y y) + z z)); a component's area =
 * the sum over its faces in ascending face order by a segmented scan of fixed shape (8 consecutive faces per lane, 256 lanes by
 * doubling steps, tiles of 2048 in order) -- not np.bincount's order, so the last bits can differ.  largest = 1: keep[f] = 1 iff f
 * lies in the component of largest area, the smallest label among equals (np.argmax's first); largest = 0: iff its component's
 * area > threshold.  Faces without a label get 0.  Workspace: adfp_mesh_component_keep_workspace_bytes(n_faces).  A NaN threshold
 * or largest outside {0, 1} is ADFP_E_ARG. */
size_t adfp_mesh_component_keep_workspace_bytes(long long n_faces);
int adfp_mesh_component_keep(const float* verts, long long n_verts, const int* faces, long long n_faces, const int* labels, int largest,
                             double threshold, unsigned char* keep, void* workspace, size_t workspace_bytes, void* stream);

/* Compaction: the faces with keep[f] != 0 in their order, the vertices they use in ascending index, the faces re-indexed.
 * _plan writes totals[2] (device long long) = (vertices, faces) that remain and keeps the positions in the workspace; the caller
 * reads the totals, allocates, and calls _emit with the same workspace and those totals (nothing is written past them). */
size_t adfp_mesh_compact_workspace_bytes(long long n_verts, long long n_faces);
int adfp_mesh_compact_plan(const int* faces, long long n_faces, long long n_verts, const unsigned char* keep, void* workspace,
                           size_t workspace_bytes, long long* totals, void* stream);
int adfp_mesh_compact_emit(const float* verts, long long n_verts, const int* faces, long long n_faces, const void* workspace,
                           size_t workspace_bytes, float* verts_out, long long n_verts_out, int* faces_out, long long n_faces_out, void* stream);

/* Coincident vertices: vertices whose three f32 bit patterns are equal (-0.0 and +0.0 differ, equal NaN patterns merge) collapse
 * into the one of lowest index; survivors keep their order.  _plan groups the vertices with six stable 16-bit passes of
 * adfp_sort_pairs over the raw words and writes *total (device long long) = the survivors; _emit writes them (and their colours
 * [V][3] uint8 when colors / colors_out are given: both or neither) and all n_faces faces re-indexed. */
size_t adfp_mesh_merge_workspace_bytes(long long n_verts);
int adfp_mesh_merge_plan(const float* verts, long long n_verts, void* workspace, size_t workspace_bytes, long long* total, void* stream);
int adfp_mesh_merge_emit(const float* verts, const unsigned char* colors, long long n_verts, const int* faces, long long n_faces,
                         const void* workspace, size_t workspace_bytes, float* verts_out, unsigned char* colors_out, long long n_verts_out,
                         int* faces_out, void* stream);

/* (np.clip(c, 0, 1) * 255).astype(np.uint8) of Mesher.py:523-524 in f32: out [n][3] bytes from rows of `stride` >= 3 floats (the
 * first three are used); NaN gives 0. */
int adfp_mesh_color_bytes(const float* rgb, long long n, int stride, unsigned char* out, void* stream);

/* ---- mesh simplification (vertex clustering: what open3d users call TriangleMesh::simplify_vertex_clustering) ----------------
 * One vertex per occupied voxel cell.  open3d is not installed where this was written and its function was never run against
 * this one: the rules below are this package's own statement of vertex clustering.  They follow open3d's cell rule and its
 * quadric accumulation as we read it; three choices are ours: the truncated placement, the dropped unreferenced clusters and
 * the output order.  Deterministic: no atomics decide anything, the same input gives the same bits.
 * Inputs: verts [V][3] f32, faces [F][3] int32, colors [V][3] uint8 or NULL (all device); voxel_size (f64, > 0, finite);
 * contraction ADFP_SIMPLIFY_AVERAGE or ADFP_SIMPLIFY_QUADRIC; min_bound, max_bound: HOST f64 [3], the exact per-axis minimum and
 * maximum of the vertices.
 * Cells: adfp_voxel_down_sample's rule on (double)verts -- vmin = min_bound - voxel_size * 0.5, N_c = floor((max_bound_c - vmin_c)
 * / voxel_size) + 1 (more than 2^21 is ADFP_E_UNSUPPORTED), i_c = floor((p_c - vmin_c) / voxel_size), key (i_0 N_1 + i_1) N_2 +
 * i_2, the vertices sorted stably by key in passes of 31 key bits from the lowest.  Cluster k = the k-th occupied cell in
 * ascending key order.
 * Average: m_k = the f64 sum of the cell's vertices in input order over their count n (each component divided).  Colour per
 * channel: (2 S + n) / (2 n) in integers (round half up), S the cell's integer sum.  Colours are these in both modes.
 * Quadric placement: for a face with vertices p0, p1, p2 in f64, g = (p1 - p0) x (p2 - p0), l = sqrt((g0 g0 + g1 g1) + g2 g2); a
 * face with l == 0 or non-finite l contributes nothing; else n = g / l, w = l / 2.  The face contributes once per corner to that
 * corner's cluster (twice to a cluster that holds two of its vertices, as open3d does): with d = -n . (p0 - m_k), A += w n n^T,
 * b += w d n, summed per cluster in ascending face index, then corner index (the 3 F contributions are generated face-major and
 * sorted stably by cluster).  With A = sum lambda_i e_i e_i^T (eight cyclic Jacobi sweeps in f64), lambda_max the largest:
 * x = sum over {i : lambda_i > 1e-3 lambda_max} of e_i (e_i . (-b)) / lambda_i -- a flat patch moves along its normal only, an
 * edge along two directions, a corner freely.  If lambda_max is not positive, or max_c |x_c| > voxel_size, the cluster keeps m_k;
 * else its position is m_k + x.  Positions are rounded to f32 once, at the end.  (Sums and products of the quadric are not
 * promised bit for bit against another evaluation order; a cluster whose lambda_i / lambda_max or max |x_c| sits at its threshold
 * can fall either way.)
 * Faces: each face maps through vertex -> cluster; a face with two equal indices is dropped; a survivor is rotated so that its
 * smallest index is first (orientation kept); among faces with the same rotated triple the earliest input face survives
 * (oppositely oriented copies are different triples: both stay); survivors keep input order.  A face with an index outside
 * [0, V) is never dereferenced: it contributes nothing and is dropped.
 * Vertices: clusters that no surviving face references are dropped, the rest keep ascending key order, faces are renumbered
 * (adfp_mesh_compact_plan on the triples, inside the workspace).
 * _plan writes totals[2] (device long long) = (vertices, faces) that remain; the caller reads them, allocates, and calls _emit with
 * the same counts, workspace and totals; colors_out may be given only when _plan had colors.  V = 0 or F = 0 writes totals (0, 0)
 * and launches nothing.  adfp_mesh_simplify_workspace_bytes(V, F): 0 for V <= 0, F <= 0 or beyond the limits.  One lane per cell
 * walks the cell's run: a voxel as large as the model is served, slowly.
 * Errors, before any launch: ADFP_E_ARG for a null pointer, a negative count, voxel_size <= 0 or non-finite, non-finite bounds or
 * min_bound > max_bound, contraction outside {0, 1}, more out than in; ADFP_E_UNSUPPORTED for V or 3 F above 2^31 - 1025 or more
 * than 2^21 cells on an axis; ADFP_E_WORKSPACE. */
#define ADFP_SIMPLIFY_AVERAGE 0
#define ADFP_SIMPLIFY_QUADRIC 1
size_t adfp_mesh_simplify_workspace_bytes(long long n_verts, long long n_faces);
int adfp_mesh_simplify_plan(const float* verts, long long n_verts, const int* faces, long long n_faces, const unsigned char* colors /*or NULL*/,
                            double voxel_size, int contraction, const double min_bound[3], const double max_bound[3], void* workspace,
                            size_t workspace_bytes, long long* totals, void* stream);
int adfp_mesh_simplify_emit(long long n_verts, long long n_faces, const void* workspace, size_t workspace_bytes, float* verts_out,
                            unsigned char* colors_out /*or NULL*/, long long n_verts_out, int* faces_out, long long n_faces_out, void* stream);

/* ---- mesh colours from the keyframes (Mesher's color_mesh_extraction_method: keyframe_projection) ---------------------------
 * Every vertex is projected into every keyframe; the keyframe's own depth image rejects the views in which the vertex is occluded
 * or falls on a hole; the surviving views are blended.  The rule below is this package's own statement: nothing of it is in the
 * reference.  One launch, no workspace.  Nothing is decided by an atomic: the same input gives the same bits every run.
 * Inputs (device unless said): verts [V][3] f32 (the Mesher's scaled world); normals [V][3] f32 or NULL; per keyframe k < K:
 * w2c [K][12] f32, formed as adfp_mesh_seen_mask's (the top three rows of np.linalg.inv of the f32 pose), center [K][3] f32 =
 * c2w[:3, 3], depth [K][H][W] f32, color [K][H][W][3] f32; fx, fy, cx, cy, depth_tol (f32, host); W, H, border >= 0, blend.
 * For vertex p = verts[i] and keyframe k, all in f32, every product and sum rounded on its own (no FMA):
 *   1. cam, X, Z, zz, u, v: adfp_mesh_seen_mask's projection, operation for operation (cam = ((w0 x + w1 y) + w2 z) + w3 per row,
 *      X = -cam.x, Z = cam.z, zz = Z + 1e-8, u = (fx X + cx Z) / zz, v = (fy cam.y + cy Z) / zz).
 *   2. in frame iff zz < 0 && border <= u <= W - 1 - border && border <= v <= H - 1 - border.  A NaN fails.
 *   3. x0 = min((int)floorf(u), W - 2), y0 = min((int)floorf(v), H - 2), ax = u - x0, ay = v - y0, z = -Z.
 *   4. visible iff each of the four depths d at (y0 + dy, x0 + dx), dx, dy in {0, 1}, has d > 0 && fabsf(d - z) <= depth_tol.  All
 *      four must agree: a footprint that straddles a depth edge is where colours bleed; one hole or one far corner drops the view.
 *   5. per channel c = ((w00 c00 + w01 c01) + w10 c10) + w11 c11, c_yx the colour at (y0 + y, x0 + x), w00 = (1 - ax)(1 - ay),
 *      w01 = ax (1 - ay), w10 = (1 - ax) ay, w11 = ax ay.
 *   6. to = center - p, dist = sqrtf((to.x to.x + to.y to.y) + to.z to.z), cosv = fabsf((to.x n.x + to.y n.y) + to.z n.z) /
 *      fmaxf(dist, 1e-12f), or 1 without normals; w = cosv / fmaxf(z z, 1e-12f).  The view contributes iff it is visible and
 *      w > 0: a zero or NaN normal contributes nothing.
 *   7. ADFP_BLEND_WEIGHTED: contributing views in ascending k: acc += w c, wsum += w; rgb = acc / wsum.
 *   8. ADFP_BLEND_BEST: the contributing view of largest w wins, a later view only if its w is strictly greater; rgb = its c,
 *      wsum = its w.
 * Outputs: rgb [V][3] f32 (zeros where no view contributes), wsum [V] f32, count [V] int32 (the contributing views, in both
 * modes), best [V] int32 (the view of largest w, the smallest index among equals; -1 if none).  V = 0 returns 0 and touches
 * nothing; K = 0 writes zeros and best = -1.
 * Errors, before any launch: ADFP_E_ARG for a null pointer (normals may be NULL; the keyframe arrays may be NULL when K = 0), a
 * negative count, H or W < 1, an unknown blend, depth_tol negative or not finite, border < 0 or 2 border > min(W, H) - 2;
 * ADFP_E_UNSUPPORTED for H or W < 2 (the footprint is 2 x 2), H or W > 32768, K > 32768, V > 2^31 - 1025. */
#define ADFP_BLEND_WEIGHTED 0
#define ADFP_BLEND_BEST     1
int adfp_mesh_project_colors(const float* verts, const float* normals /*or NULL*/, long long n_verts, const float* w2c, const float* center,
                             const float* depth, const float* color, long long n_keyframes, float fx, float fy, float cx, float cy, int W,
                             int H, float depth_tol, int border, int blend, float* rgb, float* wsum, int* count, int* best, void* stream);

/* ---- mesh bound (mesher.Mesher.get_bound_planes: the hull of the keyframes' camera centres and back-projected depth pixels) ----
 * The point work of a quickhull in rounds (mesh.depth_hull keeps the facets of the few hundred hull vertices with Qhull on the
 * host).  The scene: depth [K][H][W] (f32, device), poses [K][16] (f32, device; row-major [4,4] est_c2w), fx, fy, cx, cy (f64, host).
 * The points are never stored.  A point is named by an id (int64): id = k (H W + 1) + j; j = 0 is keyframe k's camera centre,
 * j = 1 + row W + col its pixel (row, col).  Every kernel recomputes a point from its id, all in f64, every product and sum rounded
 * on its own (no FMA), in exactly this order:
 *   pose      M = poses[k] widened to f64, columns 1 and 2 negated (the OpenCV camera of Mesher.py:250-251): R_c0 = M[c][0],
 *             R_c1 = -M[c][1], R_c2 = -M[c][2], t_c = M[c][3];
 *   validity  d = depth[k][row][col] widened to f64; the pixel is a point iff d > 0 && d < 1000 (NaN and inf fail);
 *   camera    x = ((col - cx) / fx) d,  y = ((row - cy) / fy) d,  z = d;
 *   world     p_c = ((R_c0 x + R_c1 y) + R_c2 z) + t_c;   a centre is p_c = t_c, and always a point.
 * An id outside [0, K (H W + 1)) on the device is never dereferenced: it names no point.  Plane evaluation, the same everywhere:
 * s_f = ((n_x p_x + n_y p_y) + n_z p_z) + d_f for planes [F][4] (f64, device; n, d; inside: s <= 0), and m = max_f s_f formed by
 * `s > m` from -inf in facet order.  No result depends on the order atomics land in (they are integer max / min); the same input
 * gives the same bits.  Errors: ADFP_E_ARG for a null pointer, K < 0, H or W < 1, fx or fy 0 or non-finite, cx or cy non-finite,
 * a negative count, D outside [1, ADFP_BOUND_MAX_DIRECTIONS], F < 1; ADFP_E_UNSUPPORTED for H or W > 32768 or more than 2^40 ids;
 * ADFP_E_WORKSPACE.  K = 0 (support) and n = 0 do nothing. */
#define ADFP_BOUND_MAX_DIRECTIONS 1024
/* Support pass, one pass over all ids: best_id[i] (int64, device, [D]) = the point with the largest ((u_x p_x + u_y p_y) + u_z p_z)
 * for directions[i] = u ([D][3] f64, device), the lowest id among equals, -1 when there is no point.  aabb [6] (f64, device) = the
 * minimum (x, y, z) then the maximum (x, y, z) of the points; counts [2] (device long long) = the number of points and the number
 * of NON-FINITE points (a pose with a NaN or inf produces them): those take no part in best_id, aabb or counts[0].  Workspace:
 * adfp_bound_support_workspace_bytes (per-workgroup partials, at most 1024 workgroups per 256 directions). */
size_t adfp_bound_support_workspace_bytes(long long K, int H, int W, int D);
int adfp_bound_support(const float* depth, const float* poses, long long K, int H, int W, double fx, double fy, double cx, double cy,
                       const double* directions, int D, void* workspace, size_t workspace_bytes, long long* best_id, double* aabb,
                       long long* counts, void* stream);
/* One round: candidate i of n_in is ids_in[i] (int64, device, ascending), or id i itself when ids_in is NULL (then n_in must be
 * K (H W + 1)).  A candidate that is no point, or whose m <= eps, is dropped.  The others (the survivors) go to ids_out in
 * ascending position (so ascending id); *count (device long long) = their number, of which only the first ids_cap are written: the
 * caller compares.  Each survivor is assigned to the LOWEST facet that attains its m; far_dist[f] (f64, device) = the largest m
 * over the survivors assigned to f among the first ids_cap (0 when none), far_id[f] (int64) the lowest id that attains it (-1 when
 * none).  Planes beyond what the LDS of a workgroup holds are taken in chunks inside the launch.  eps must be finite and >= 0.
 * Workspace: adfp_bound_classify_workspace_bytes(n_in) = one bit per candidate and 12 bytes per tile of 1024. */
size_t adfp_bound_classify_workspace_bytes(long long n_in);
int adfp_bound_classify(const float* depth, const float* poses, long long K, int H, int W, double fx, double fy, double cx, double cy,
                        const long long* ids_in, long long n_in, const double* planes, int F, double eps, void* workspace,
                        size_t workspace_bytes, long long* ids_out, long long ids_cap, long long* count, long long* far_id, double* far_dist,
                        void* stream);
/* out [n][3] (f64, device) = the points of ids [n] (int64, device); NaN for an id that names no point. */
int adfp_bound_points(const float* depth, const float* poses, long long K, int H, int W, double fx, double fy, double cx, double cy,
                      const long long* ids, long long n, double* out, void* stream);

/* ---- frame ingestion (datasets.FrameIngest: the reference's BaseDataset.__getitem__, src/utils/datasets.py:77-113) ----
 * The decoded images go in as they are -- colour [color_h][color_w][3] uint8, depth [depth_h][depth_w] uint16 or f32, both on the
 * device -- and ONE launch writes, for each of n_jobs frames, color_out [H][W][3] (f32 or f64) and depth_out [H][W] (f32), H and W
 * as adfp_ingest_out_shape gives them.  Per output pixel, nothing rounded that the reference does not round, no FMA:
 *   A  colour   c = byte / 255 in f64; channel order RGB (color_order 0 reads the bytes as B, G, R).
 *   B  resize   only when (color_h, color_w) != (depth_h, depth_w): cv2.resize(img_f64, (depth_w, depth_h)), i.e. bilinear with
 *               half-pixel centres and float coefficients: fx = (float)((dx + 0.5) * (double)color_w / depth_w - 0.5), sx = floor(fx),
 *               fx -= sx (float); sx < 0 gives sx = 0, fx = 0; sx >= color_w - 1 gives sx = color_w - 1, fx = 0; weights 1.f - fx and
 *               fx widened to f64.  In y the same coefficients, the two rows sy and sy + 1 clamped into the image and their weights
 *               kept.  OpenCV itself forms scale = 1. / ((double)depth_w / color_w) and (dx + 0.5) * scale - 0.5; the float
 *               coefficients of the two forms are equal for 1296 -> 640, 968 -> 480 and the tests' shapes (compared on the
 *               host), and a last-bit f64 difference survives the rounding to float only at a rounding tie; parity with
 *               cv2.resize itself is checked only where cv2 is installed (tests/test_ingest_host.py).  Horizontal pass first: h_r = S[r][sx] w0 + S[r][sx + 1] w1 for both rows, then h_0 b0 + h_1 b1, all f64.
 *   C  crop_size  only when crop_h, crop_w != 0, on the result of B: colour as F.interpolate(bilinear, align_corners=True) forms
 *               it for f64 on the CPU (ratio = (in - 1) / (out - 1) in f64, i0 = (int)(ratio d), l1 = ratio d - i0, l0 = 1 - l1,
 *               ((w00 v00 + w01 v01) + w10 v10) + w11 v11 with w_ab = l_a(y) l_b(x); equal sizes copy); depth as
 *               F.interpolate(nearest): src = min((int)floorf(d * ((float)in / out)), in - 1).
 *   D  edge     [crop_edge : -crop_edge] in both axes of the result of C.
 *   depth       ((float)raw / png_depth_scale) * scale: two f32 roundings; depth_kind 1 takes raw as the f32 it is.
 *   colour out  the f64 value, or its single rounding to f32.
 * The jobs are a HOST array (copied into the kernel's arguments, like adfp_sample_keyframes' frames).  Errors, before any launch:
 * ADFP_E_ARG for a null geom / jobs / job pointer, a size < 1, crop_h or crop_w negative or only one of them 0, crop_edge < 0 or
 * 2 crop_edge >= the height or width it crops, png_depth_scale 0 or non-finite, an unknown color_order / depth_kind / color_out,
 * n_jobs < 0; ADFP_E_UNSUPPORTED for n_jobs > ADFP_INGEST_MAX_JOBS or a size above 32768.  n_jobs = 0 launches nothing. */
#define ADFP_INGEST_MAX_JOBS 16
typedef struct adfp_ingest_geom {           /* host */
    int color_h, color_w;                   /* decoded colour image */
    int depth_h, depth_w;                   /* decoded depth image */
    int crop_h, crop_w;                     /* cfg cam.crop_size, 0 0 = none */
    int crop_edge;                          /* cfg cam.crop_edge */
    int color_order;                        /* 0 = BGR (cv2.imread), 1 = RGB (PIL) */
    int depth_kind;                         /* 0 = uint16, 1 = float32 */
    int color_out;                          /* 0 = float32, 1 = float64 (the reference's dtype) */
    float png_depth_scale, scale;
} adfp_ingest_geom;
typedef struct adfp_ingest_job { const unsigned char* color; const void* depth; void* color_out; float* depth_out; } adfp_ingest_job;
int adfp_ingest_frames(const adfp_ingest_geom* geom, int n_jobs, const adfp_ingest_job* jobs /*host*/, void* stream);
int adfp_ingest_out_shape(const adfp_ingest_geom* geom, int* H, int* W);    /* host only */

/* ---- lens undistortion (cfg cam.distortion), stage U in front of stage A of frame ingestion ----
 * This package's own statement of the scheme of cv2.undistort(img, K, dist) with newCameraMatrix = K: a 1/32-pixel fixed-point
 * map, bilinear taps, constant border 0.  It has NOT been compared with cv2 (not a dependency, not installed where this was
 * written): no byte parity with cv2 is claimed.  tests/undistort_ref.py states the rule in numpy.
 *
 * Map: one int32 pair (iu, iv) per pixel (u, v) of the decoded colour image [color_h][color_w], all in f64, in this operation
 * order, no FMA; dist = k1 k2 p1 p2 [k3 [k4 k5 k6]] (4, 5 or 8 coefficients, the missing ones 0):
 *   x = (u - cx) / fx;  y = (v - cy) / fy;  r2 = x*x + y*y
 *   kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2)
 *   xd = x*kr + p1*(2*x*y) + p2*(r2 + 2*(x*x));   yd = y*kr + p1*(r2 + 2*(y*y)) + p2*(2*x*y)
 *   U = fx*xd + cx;  V = fy*yd + cy
 *   iu = rint(clamp(32*U, -2^30, 2^30)), iv likewise (nearest-even; clamped BEFORE the conversion to int)
 *   a non-finite U or V gives (INT32_MIN, INT32_MIN)
 * Remap, all integer: sx = iu >> 5, sy = iv >> 5 (arithmetic), a = iu & 31, b = iv & 31; taps p00 = S[sy][sx], p01 = S[sy][sx+1],
 * p10 = S[sy+1][sx], p11 = S[sy+1][sx+1] per channel, a tap outside [0, color_h) x [0, color_w) contributing 0;
 *   byte = ((32-a)(32-b) p00 + a(32-b) p01 + (32-a)b p10 + ab p11 + 512) >> 10
 * (the weights sum to 1024).  The sentinel entry gives 0, as every entry whose taps all lie outside.
 *
 * adfp_undistort_map: host only, once per dataset and colour size; map is a HOST array [color_h][color_w][2].  ADFP_E_ARG for a
 * null pointer, a size < 1, fx or fy 0 or non-finite, cx or cy non-finite; ADFP_E_UNSUPPORTED for n_dist outside {4, 5, 8} or a
 * size above 32768.
 * adfp_ingest_frames_undistort: adfp_ingest_frames with the byte above standing where stage A reads a source byte; stages A-D and
 * the depth path are untouched, no intermediate image exists.  map is a DEVICE array [color_h][color_w][2], 8-byte aligned
 * (otherwise ADFP_E_ARG); a NULL map is adfp_ingest_frames exactly.  Errors as adfp_ingest_frames.
 * adfp_undistort_image: dst [h][w][3] uint8 = the remap of src [h][w][3] through map [h][w][2] (all device; dst must not overlap
 * src); the channel order is kept.  ADFP_E_ARG for a null pointer, a misaligned map, h or w < 1; ADFP_E_UNSUPPORTED above 32768. */
int adfp_undistort_map(int color_h, int color_w, double fx, double fy, double cx, double cy, const double* dist, int n_dist,
                       int* map /*host [color_h][color_w][2]*/);
int adfp_ingest_frames_undistort(const adfp_ingest_geom* geom, const int* map /*device [color_h][color_w][2]*/, int n_jobs,
                                 const adfp_ingest_job* jobs /*host*/, void* stream);
int adfp_undistort_image(const unsigned char* src, const int* map, int h, int w, unsigned char* dst, void* stream);

/* ---- visualisation (visualizer.Visualizer: the reference's src/utils/Visualizer.py:71-114, everything after render_img) ----
 * The frame's input images -- gt_depth [H][W] f32, gt_color [H][W][3] f32 or f64 (gt_color_f64) -- and the rendered ones -- depth
 * [H][W] f64, color [H][W][3] f32 -- go in as they lie in device memory, and two launches write the uint8 canvas [rows][cols][3]
 * of six panels and stats [ADFP_VIS_STATS] (f64, device).  The contract is what matplotlib maps a data array to (Normalize,
 * Colormap.__call__, the float-RGB rule of imshow), not what imshow resamples into a figure; tests/vis_ref.py states it in numpy.
 *   layout     h = ceil(H / stride), w = ceil(W / stride); rows = 2 h + 3 gap, cols = 3 w + 4 gap; the background is white (255).
 *              Panel (r, k) has its top-left corner at (gap + r (h + gap), gap + k (w + gap)); its pixel (i, j) shows source
 *              pixel (i stride, j stride).  Row 0: input depth, generated depth, depth residual; row 1: input RGB, generated
 *              RGB, RGB residual.
 *   residuals  depth: |(double)gt_depth - depth|, 0 where gt_depth == 0.  RGB: |gt_color - color| in the promoted dtype (f32 with
 *              f32 gt_color, f64 with f64), all three channels 0 where gt_depth == 0.
 *   depth panels  vmax = max(gt_depth), an f32 (gt_depth is taken to be free of NaN).  x = v / vmax, in f32 for the input-depth
 *              panel and in f64 with (double)vmax for the other two; the division is IEEE.  index = 255 if 256 x == 256, else
 *              trunc(256 x) clamped to [0, 255]; the colour is entry `index` of matplotlib's 'plasma' as bytes.  NaN is white.
 *              vmax == 0 maps every value to index 0.  (vmax < 0, where matplotlib raises, takes the same formula.)
 *   RGB panels    byte = trunc(255 clip(v, 0, 1)), the product in the array's own dtype; NaN is 0.
 *   stats      over the full-resolution frame whatever the stride: [0] vmax; [1] n_valid, the pixels with gt_depth > 0 and finite
 *              rendered depth and colour (all three channels); [2] depth_abs_sum, the depth residual summed over those; [3]
 *              color_sq_sum, ((double)gt_color - (double)color)^2 summed over the three channels of every pixel with finite
 *              rendered colour; [4] n_nonfinite, the pixels whose rendered depth or colour is not finite; [5] n_color, the
 *              pixels color_sq_sum counted (a pixel may have a finite colour beside a NaN depth, so [4] does not give it).
 *              Sums are f64; per-workgroup partials over a grid that depends on H W alone, then one fixed-order pass: no float
 *              atomics, the same bits on every call.
 * Asynchronous on `stream`, no allocation, no pointer kept; nothing is read back between the two launches (vmax reaches the
 * second through the workspace).  Workspace: adfp_vis_workspace_bytes(geom) (0 for a bad geometry), 8-byte aligned.  Errors,
 * before any launch: ADFP_E_ARG for a null pointer, H, W or stride < 1, gap < 0, gt_color_f64 outside {0, 1}, a workspace that is
 * too small or misaligned; ADFP_E_UNSUPPORTED for H, W or gap above 32768. */
#define ADFP_VIS_STATS 6
typedef struct adfp_vis_geom {              /* host */
    int H, W;                               /* the frame */
    int stride;                             /* every stride-th source pixel in both axes */
    int gap;                                /* gutter and margin, canvas pixels */
    int gt_color_f64;                       /* gt_color: 0 = float32, 1 = float64 (the reference's dtype) */
} adfp_vis_geom;
int adfp_vis_canvas_shape(const adfp_vis_geom* geom, int* rows, int* cols);    /* host only */
size_t adfp_vis_workspace_bytes(const adfp_vis_geom* geom);
int adfp_vis_panels(const adfp_vis_geom* geom, const float* gt_depth, const void* gt_color, const double* depth, const float* color,
                    unsigned char* canvas, double* stats, void* workspace, size_t workspace_bytes, void* stream);

/* ---- rendering metrics (render_eval.FrameMetrics: PSNR, SSIM, MS-SSIM and depth L1 of a rendered frame; no counterpart in the
 * reference) ----
 * One frame's inputs are adfp_vis_panels' -- gt_depth [H][W] f32, gt_color [H][W][3] f32 or f64 (gt_color_f64), and the rendered
 * depth [H][W] f64 and color [H][W][3] f32 as render_img returns them -- read as they lie in device memory.  The output is one
 * row of ADFP_FRAME_METRICS doubles at a device address the caller chooses, so that a run fills a table [n_frames][35] without a
 * read-back per frame.  tests/render_ref.py states the contract in numpy.
 *   row[0..4]  n_valid, depth_abs_sum, color_sq_sum, n_color, n_nonfinite: over the full-resolution frame; n_valid, the pixels with
 *              gt_depth > 0 and finite rendered depth and colour (all three channels); depth_abs_sum, the depth residual
 *              |(double)gt_depth - depth| summed over those; color_sq_sum, ((double)gt_color - (double)color)^2 summed over the
 *              three channels of every pixel with finite rendered colour; n_color, the pixels color_sq_sum counted; n_nonfinite,
 *              the pixels whose rendered depth or colour is not finite.  These are adfp_vis_panels' stats of the same names, over
 *              the same reduction grid and in the same order: the same bits.
 *   row[5 + 6 k + 2 c], row[5 + 6 k + 2 c + 1]   for level k in 0..4 and channel c in 0..2: the sum over all window positions of
 *              the SSIM map and of the contrast-structure map of that level and channel.  Levels at or beyond geom.levels hold
 *              exactly 0.
 *   images     the whole image; gt_depth plays no part.  x = gt_color, y = clip(color, 0, 1) with NaN mapped to 0 (the RGB
 *              panel's rule), both taken to double.
 *   level 0    window: 11 taps, Gaussian, sigma 1.5, normalised to sum 1 in f64, applied separably with no padding: level k of
 *              size Hk x Wk has (Hk - 10)(Wk - 10) positions.  Per position mx, my, sxx = E[x^2] - mx^2, syy, sxy; C1 = 1e-4,
 *              C2 = 9e-4 (data range 1); cs = (2 sxy + C2) / (sxx + syy + C2); ssim = (2 mx my + C1) / (mx^2 + my^2 + C1) * cs.
 *              All arithmetic is f64.
 *   level k+1  level k averaged over 2 x 2 blocks with stride 2 after zero padding of Hk mod 2 rows and Wk mod 2 columns on each
 *              side; the padded zeros count in the average (torch's avg_pool2d(x, 2, padding=(Hk % 2, Wk % 2))), so the size is
 *              floor((Hk + 2 (Hk mod 2) - 2) / 2) + 1.  The pooled images are f64.
 *   This is the convention of the pytorch_msssim package.  The numbers are held to the formula as restated in
 *   tests/render_ref.py (and, independently, in torch f64 by tests/test_render_ref_host.py), NOT to that package or to skimage:
 *   neither has been compared with.
 *   sums       f64; per-workgroup partials over grids that depend on the geometry alone, then one pass in fixed order: no float
 *              atomics, the same bits on every call.
 * Asynchronous on `stream`, no allocation, no pointer kept, nothing read back between the launches (2 + 2 levels - 1 of them for
 * levels >= 1); capturable in a graph.  Workspace: adfp_frame_metrics_workspace_bytes(geom) (0 for a bad geometry).  Errors, all
 * before any launch: ADFP_E_ARG for a null pointer, H or W < 1, levels outside 0..5, gt_color_f64 outside {0, 1}, a level
 * k < levels whose image is smaller than 11 on a side, a row or workspace that is not 8-byte aligned, a workspace that is too
 * small; ADFP_E_UNSUPPORTED for H or W above 32768. */
#define ADFP_FRAME_METRICS 35
typedef struct adfp_metrics_geom {          /* host */
    int H, W;                               /* the frame */
    int levels;                             /* 0..5; 0 = entries [0..4] only */
    int gt_color_f64;                       /* gt_color: 0 = float32, 1 = float64 (the reference's dtype) */
} adfp_metrics_geom;
size_t adfp_frame_metrics_workspace_bytes(const adfp_metrics_geom* geom);      /* 0 for a bad geometry */
int adfp_frame_metrics_windows(const adfp_metrics_geom* geom, long long windows[5]);   /* host only: positions per level, 0 beyond levels */
int adfp_frame_metrics(const adfp_metrics_geom* geom, const float* gt_depth, const void* gt_color, const double* depth,
                       const float* color, double* row /* device [ADFP_FRAME_METRICS] */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- TSDF raycast (tsdf_raycast.TsdfRaycaster, Renderer.render_novel: the depth image of the TSDF prior from any pose; no
 * counterpart in the reference, whose render_img needs a sensor depth image, src/utils/Renderer.py:292) ----
 * depth [V][H][W] f32: per pixel the z-depth of the first + -> - crossing of the TSDF along the pixel's ray, 0 where there is none
 * (what the sampler reads as "no sensor depth").  tests/tsdfcast_ref.py states the rule in torch:
 *   ray      adfp_get_rays' (f32, direction with camera z = -1, so the ray parameter is the sensor depth), promoted to f64.
 *   interval tn, tf = the slab entry and exit against tsdf_bnds in f64 (an axis with d = 0 only says inside or outside);
 *            tn = max(tn, near, 0); tf = min(tf, far) when far > 0; tf < tn gives 0.
 *   march    dt = step / |d| (step in metres); sample k at t_k = tn + k dt, computed and not accumulated, while t_k <= tf; position
 *            o + d t_k in f64, normalised into tsdf_bnds in f64, then .float(), then the trilinear lookup of adfp_sample_tsdf
 *            (grid_sample, border padding, align_corners).  tsdf->corner_blocks, when given, is read instead: the same bits.
 *   hit      the first sample with f <= 0 ends the ray: depth 0 if k = 0 (the ray starts behind a surface), else
 *            t_{k-1} + dt f_{k-1} / (f_{k-1} - f_k) in f64, stored as f32.  No band test on f_{k-1}: the rule is on interpolated
 *            values, as KinectFusion's is, so a ray that reaches a surface from behind through unobserved space (f = -1) reports
 *            a crossing at the truncation boundary.
 * Empty-space skip: adfp_tsdf_bricks_build writes a bitmap with one bit per brick of 8^3 voxels (brick (bx nby + by) nbz + bz with
 * nb = ceil(size / 8), 32 per word), set when any voxel of the brick -- padded by one voxel on every side, clipped to the volume --
 * is not >= 2^-100 (every value <= 0, and NaN).  The march passes over samples whose eight corners are vouched positive without
 * looking them up; because t_k is computed from k, the image is byte for byte the image with ADFP_CAST_NO_SKIP
 * (csrc/adfp_tsdfcast.h argues it).  Build the bitmap once per volume and again after the volume changes.
 * lookups (device, or NULL): the number of trilinear lookups of the call is ADDED to it (a diagnostic: one atomic per pixel).
 * Asynchronous on `stream`, no allocation, no pointer kept; one launch each.  Errors, all before any launch: ADFP_E_ARG for a null
 * pointer (bricks may be NULL with ADFP_CAST_NO_SKIP), a size or V, H, W < 1, step <= 0 or NaN, NaN near or far, an empty bound, an
 * unknown option bit, a bitmap that is unaligned or smaller than adfp_tsdf_bricks_bytes; ADFP_E_UNSUPPORTED for a volume side, H or
 * W above 32768, V above 65535, or a step below 2^-24 of the bound's diagonal.  adfp_tsdf_bricks_bytes is 0 for a bad size. */
#define ADFP_CAST_NO_SKIP 1      /* options bit: look every sample up */
size_t adfp_tsdf_bricks_bytes(int Z, int Y, int X);
int adfp_tsdf_bricks_build(const adfp_tsdf* tsdf /*host*/, void* bricks, size_t bricks_bytes, void* stream);
int adfp_tsdf_raycast(const adfp_tsdf* tsdf /*host*/, const double tsdf_bnds[3][2] /*host*/, const void* bricks, size_t bricks_bytes,
                      const float* c2w /*[V][4][4]*/, int V, int H, int W, float fx, float fy, float cx, float cy, double near, double far,
                      double step, int options, float* depth /*[V][H][W]*/, unsigned long long* lookups, void* stream);

/* ---- Depth ICP (icp.DepthICP, tracking.init: icp: KinectFusion's frame-to-model point-to-plane ICP over the whole depth image, the
 * sensor depth against the raycast of the TSDF prior; no counterpart in the reference) ----  tests/icp_ref.py states the rule in numpy.
 * Camera convention: adfp_get_rays'.  Pixel (u, v) with depth d is the camera point V = ((u - cx) / fx d, -(v - cy) / fy d, -d); d <= 0
 * or non-finite is invalid.  Vertices are never stored, they are recomputed from the depth.  fx, fy, cx, cy are f32 values; all
 * arithmetic below is f64 on f32 loads.
 * Normal map (adfp_depth_normals, one launch for V images): a = V(v, u + 1) - V(v, u), b = V(v + 1, u) - V(v, u), n = normalize(b x a),
 *   negated when n . V(v, u) > 0.  n = 0 (invalid) on the last row and column, when any of the three depths is invalid, when |b x a| = 0,
 *   and, with max_jump > 0, when either neighbour's depth differs from the pixel's by more than max_jump.  normals [V][H][W][3] f32.
 * One step (adfp_icp_step; T is the f64 camera-to-world estimate in the state block, p_ref the f32 pose the model maps were raycast
 *   from).  For every sensor pixel with u % stride == 0, v % stride == 0 and a valid normal N_s:
 *     x = T V_s, n_s = R_T N_s;  x_c = R_ref^T (x - t_ref), z = -x_c.z, required > 0;
 *     u' = floor(fx x_c.x / z + cx + 0.5), v' = floor(-fy x_c.y / z + cy + 0.5), required inside the image with a valid model normal;
 *     m = p_ref V_m(u', v'), n = R_ref N_m(u', v');  the pair is kept if |x - m| <= dist_tol and n_s . n >= cos_tol.
 *   Per pair r = n . (m - x), J = [x x n, n] for the twist xi = (w, t) applied on the left (x <- x + w x x + t).  The ADFP_ICP_SUMS = 29
 *   f64 sums, in this order: the 21 upper entries of sum J^T J row by row, the 6 of sum J^T r, sum r^2, the pair count.  They are
 *   added in an order fixed by the launch geometry (no atomics): the same inputs give the same bytes.
 *   Solve: pairs < min_pairs (a count) gives ADFP_ICP_FEW_PAIRS.  Otherwise LDL^T without pivoting, pivots d_0 .. d_5 in turn; the
 *   first d_j that is not > min_pivot max diag(A) stops it with ADFP_ICP_DEGENERATE.  In either case T stays and every later step
 *   of the bracket does nothing but write its stats row (zeros and the status).  Otherwise T <- Exp(xi) T with the closed-form SE(3)
 *   exponential (R = I + A K + B K^2, translation (I + B K + C K^2) t, A = sin th / th, B = (1 - cos th) / th^2, C = (1 - A) / th^2;
 *   below th = |w| = 1e-12 the series R = I + K, I + K / 2).
 *   stats row (ADFP_ICP_STATS = 6 doubles): pairs, rmse before the update (sqrt(sum r^2 / pairs), 0 without pairs), the smallest pivot
 *   ratio d_j / max diag(A) over the pivots computed, |w|, |t|, status.  sums (device [29], or NULL) receives the step's sums.
 * Bracket: adfp_icp_begin sets T = guess (device [16] f32) and status OK.  adfp_icp_end: with status OK, shift = |t_T - t_guess| and
 *   angle = atan2(|vee(D - D^T)| / 2, (tr D - 1) / 2) of D = R_T R_guess^T; shift > max_shift or angle > max_angle (or NaN) gives
 *   ADFP_ICP_REJECTED.  c2w_out [16] f32 is T rounded (last row 0 0 0 1) when the status is OK, else the guess's own bits; cam_out [7]
 *   f32 is common.get_tensor_from_camera of c2w_out in f64 (columns normalised, negated for a negative determinant, the trace branch
 *   or the largest-diagonal branch, unit length, r >= 0): quaternion r, i, j, k, then the translation.  Its stats row, when stats is
 *   given: 0, 0, 0, angle, shift, the final status.
 * state: ADFP_ICP_STATE_BYTES of device memory, 8-byte aligned, the caller's; nothing else persists between the calls.  workspace:
 * adfp_icp_workspace_bytes(H, W) (0 for H or W outside [1, 32768]), 8-byte aligned.  Asynchronous on `stream`, no allocation, no
 * pointer kept, no read-back, graph-capturable; adfp_icp_step is two launches, the others one.  Errors, all before any launch:
 * ADFP_E_ARG for a null pointer (sums, and adfp_icp_end's stats, may be NULL), V, H, W or stride < 1, a NaN tolerance or intrinsic,
 * fx or fy 0, a misaligned block, a workspace below adfp_icp_workspace_bytes, a stats row outside [0, stats_rows);
 * ADFP_E_UNSUPPORTED for H or W above 32768 or V above 65535. */
#define ADFP_ICP_SUMS 29
#define ADFP_ICP_STATS 6
#define ADFP_ICP_STATE_BYTES 272
#define ADFP_ICP_OK 0
#define ADFP_ICP_FEW_PAIRS 1
#define ADFP_ICP_DEGENERATE 2
#define ADFP_ICP_REJECTED 3
size_t adfp_icp_workspace_bytes(int H, int W);
int adfp_depth_normals(const float* depth /*[V][H][W]*/, int V, int H, int W, float fx, float fy, float cx, float cy, float max_jump,
                       float* normals /*[V][H][W][3]*/, void* stream);
int adfp_icp_begin(const float* guess /*[16]*/, void* state, void* stream);
int adfp_icp_step(const float* depth_s, const float* normals_s, const float* depth_m, const float* normals_m, const float* p_ref /*[16]*/,
                  int H, int W, float fx, float fy, float cx, float cy, int stride, double dist_tol, double cos_tol, double min_pivot,
                  double min_pairs, void* state, double* stats /*[stats_rows][6]*/, int stats_rows, int row, double* sums /*[29] or NULL*/,
                  void* workspace, size_t workspace_bytes, void* stream);
int adfp_icp_end(void* state, double max_shift, double max_angle, float* c2w_out /*[16]*/, float* cam_out /*[7]*/,
                 double* stats /*or NULL*/, int stats_rows, int row, void* stream);

/* ---- RGB-D ICP (icp.RgbdICP, tracking.icp_rgb: the depth ICP's step with a photometric term against the last tracked frame, the
 * "keyframe" -- its sensor colour, its sensor depth, its final pose -- added to the same normal equations, as Kintinuous,
 * ElasticFusion and DVO pair the two; no counterpart in the reference) ----  tests/rgbd_icp_ref.py states the rule in numpy.
 * Conventions are "Depth ICP"'s: the camera point V(u, v, d), f64 arithmetic on f32 loads, a depth is valid when d > 0 and finite.
 * Every gate is written as !(... <= ...), so a NaN drops the pair.
 * Frame map (adfp_rgbd_frame_map, one launch): colour [H][W][3] f32 (0..1) and depth [H][W] f32 -> map [H][W][4] f32 = (I, gx, gy, d).
 *   I = (0.299 r + 0.587 g) + 0.114 b in f64; gx = (I(u + 1, v) - I(u - 1, v)) / 2 and gy = (I(u, v + 1) - I(u, v - 1)) / 2 from the
 *   UNROUNDED f64 intensities, one rounding at the store; gx = 0 in the first and the last column, gy = 0 in the first and the last
 *   row; d is the depth's own bits.  A NaN colour gives a NaN.  The 16-byte texel makes each pixel of a bilinear footprint one load.
 * Photometric pairs of a step.  T is the estimate, p_key (f32 [16]) the keyframe's pose, key its map, cur the current frame's map.
 *   For every pixel with u % stride == 0, v % stride == 0, a valid d_s = cur.d and a finite I_s = cur.I (no sensor normal is needed):
 *     x = T V_s;  y = R_key^T (x - t_key);  z = -y.z, required > 0;
 *     a = (fx y.x) / z + cx, b = (-fy y.y) / z + cy;  u0 = floor(a), v0 = floor(b), required 1 <= u0 <= W - 3 and 1 <= v0 <= H - 3 (all
 *     four footprint pixels carry central differences);  s = a - u0, t = b - v0;
 *     each of the four keyframe texels M_ji = key(v0 + j, u0 + i) needs a valid depth with |d_key - z| <= dist_tol (the occlusion gate);
 *     (I, gx, gy) = ((1-s)(1-t) M_00 + s(1-t) M_01) + ((1-s) t M_10 + s t M_11), in that order of addition;
 *     r = I_s - I, kept if |r| <= rgb_tol;
 *     c = ((gx fx) / z, -(gy fy) / z, ((gx fx) y.x - (gy fy) y.y) / z^2);  n = R_key c;  J = [x x n, n], the point-to-plane form for the
 *     same left twist.
 * Sums (ADFP_RGBD_SUMS = 31 f64): the 21 upper entries of sum_g J J^T + w sum_p J J^T, the 6 of sum_g J r + w sum_p J r, then sum r_g^2,
 *   the geometric pair count, sum r_p^2, the photometric pair count (the last four unweighted).  w = rgb_weight >= 0; a photometric
 *   pair adds w (J_i J_j) and w (J_i r).  Geometric pairs follow adfp_icp_step's rule exactly (the sensor depth is cur's fourth
 *   channel); per pixel the geometric contribution is added first.  With w = 0 or key_map NULL no photometric pair is evaluated, sums
 *   29 and 30 are 0, and sums 0..28 are adfp_icp_step's bytes on the same inputs (same grid, same order of addition).
 * Solve: max(geometric pairs, photometric pairs) < min_pairs gives ADFP_ICP_FEW_PAIRS; otherwise adfp_icp_step's LDL^T, min_pivot
 *   gate, Exp and state block.  adfp_icp_begin and adfp_icp_end bracket the steps unchanged.  The stats row keeps its meaning (pairs
 *   and rmse are the geometric ones); rgb_stats [stats_rows][ADFP_RGBD_STATS = 2] receives (photometric pairs, photometric rmse) in
 *   the same row, zeros from a step after a failed one.  sums (device [31], or NULL) receives the step's sums.
 * workspace: adfp_rgbd_workspace_bytes(H, W) = the workgroups of adfp_icp_workspace_bytes x 31 x 8 (0 for H or W outside [1, 32768]).
 * Asynchronous on `stream`, no allocation, no pointer kept, no read-back, graph-capturable; adfp_rgbd_step is two launches.  Errors,
 * all before any launch: ADFP_E_ARG for a null pointer (sums may be NULL; key_map and p_key are both given or both NULL), a map that
 * is not 16-byte aligned, a block that is not 8-byte aligned, a NaN or negative rgb_weight, a NaN rgb_tol, tolerance or intrinsic, fx
 * or fy 0, H, W or stride < 1, a workspace below adfp_rgbd_workspace_bytes, a stats row outside [0, stats_rows); ADFP_E_UNSUPPORTED
 * for H or W above 32768. */
#define ADFP_RGBD_SUMS 31
#define ADFP_RGBD_STATS 2
size_t adfp_rgbd_workspace_bytes(int H, int W);
int adfp_rgbd_frame_map(const float* color /*[H][W][3]*/, const float* depth /*[H][W]*/, int H, int W, float* map /*[H][W][4], 16-byte aligned*/,
                        void* stream);
int adfp_rgbd_step(const float* cur_map, const float* normals_s, const float* depth_m, const float* normals_m, const float* p_ref /*[16]*/,
                   const float* key_map /*or NULL*/, const float* p_key /*[16], NULL iff key_map is*/, int H, int W, float fx, float fy, float cx,
                   float cy, int stride, double dist_tol, double cos_tol, double rgb_weight, double rgb_tol, double min_pivot, double min_pairs,
                   void* state, double* stats /*[stats_rows][6]*/, double* rgb_stats /*[stats_rows][2]*/, int stats_rows, int row,
                   double* sums /*[31] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Depth bilateral filter (icp.depth_bilateral, DepthICP(bilateral=...), tracking.icp.bilateral: the filter of the raw sensor depth
 * that KinectFusion's pipeline starts with, ahead of the normal map; no counterpart in the reference) ----  tests/depth_filter_ref.py
 * states the rule in numpy.  Conventions are "Depth ICP"'s: f64 arithmetic on f32 loads, a depth is valid when d > 0 and finite.
 * For a pixel p = (u, v) of image k with an invalid depth d_p, out = +0.0f: holes are not filled.  With a valid d_p:
 *     s_p = sigma_depth + sigma_depth_z2 (d_p d_p);  a = 1 / ((2 sigma_space) sigma_space);  b = 1 / ((2 s_p) s_p);
 *     q runs over the (2 radius + 1)^2 window around p clipped to the image, rows ascending, within a row columns ascending; a q takes
 *     part when d_q is valid and !(|d_q - d_p| > 3 s_p);  w_q = exp(-((du du + dv dv) a + ((d_q - d_p) (d_q - d_p)) b)) with the integer
 *     offsets du, dv: one f64 exp per tap;  num = sum w_q d_q, den = sum w_q, both added in q's order;  out = (float)(num / den).
 *   The centre's own weight is 1, so den >= 1.  sigma_depth_z2 > 0 widens the range term with the square of the depth, as the axial
 *   noise of a structured-light or time-of-flight sensor grows.
 * One launch, no atomics: the same inputs give the same bytes.  Asynchronous on `stream`, no allocation, no pointer kept, no
 * read-back, graph-capturable.  Errors, all before any launch: ADFP_E_ARG for a null pointer, out == depth, V, H, W or radius < 1, a
 * NaN or <= 0 sigma_space or sigma_depth, a NaN or < 0 sigma_depth_z2; ADFP_E_UNSUPPORTED for radius above 8, H or W above 32768, V
 * above 65535. */
int adfp_depth_bilateral(const float* depth /*[V][H][W]*/, int V, int H, int W, int radius, double sigma_space, double sigma_depth,
                         double sigma_depth_z2, float* out /*[V][H][W]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADFP_H */
