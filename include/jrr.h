/*
 * jrr.h -- C ABI of the MI355X (gfx950) pose-refinement hot path.
 *
 * Drop-in boundary for the inner loop of the reference's scripts/optimize.py
 * (ubc-vision/joint-regressor-refinement).  The reference has no FFI layer: its boundary is
 * Python-level.  Each entry point below names the reference
 * interface (file:line in /root/reference) whose arithmetic it replaces; the Python host
 * code in joint-regressor-refinement_amd/ binds these through ctypes.
 *
 * Conventions
 *  - plain pointers and sizes only; no torch / C++ types cross the boundary.
 *  - every `*_dev` pointer is device memory owned by the caller (PyTorch's allocator), 16-byte aligned (whole
 *    tensors and pose-granular contiguous slices of them are);
 *    every `*_host` pointer is host memory read synchronously during the call.
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *    kernels are enqueued on it, no entry point synchronises the device unless stated.  (jrr_refine_run* may put part of an iteration on an engine-owned side stream, forked from and joined back into `stream` by events within the call: ordering as seen from `stream` is unchanged.)
 *  - return value: 0 on success, negative jrr_status otherwise; nothing throws.
 *  - one caller thread per engine; engines on different devices/processes are independent.
 *  - all floating point is IEEE fp32 (the reference runs `.float()`, optimize.py:160);
 *    matrix products use the exact-fp32 MFMA v_mfma_f32_32x32x2_f32.
 */
#ifndef JRR_H
#define JRR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  JRR_OK = 0,
  JRR_ERR_ARG = -1,       /* null pointer / bad size */
  JRR_ERR_HIP = -2,       /* a HIP runtime call failed; see jrr_last_error() */
  JRR_ERR_WORKSPACE = -3, /* workspace too small */
  JRR_ERR_STATE = -4,     /* engine not configured for the requested op */
  JRR_ERR_SEGMENT = -5    /* jrr_bootstrap_sums: a segment with a negative count, or one that leaves the unit table */
} jrr_status;

enum {
  JRR_NUM_VERTS = 6890,
  JRR_NUM_JOINTS = 24,
  JRR_NUM_H36M = 17,
  JRR_NUM_BETAS = 10,
  JRR_POSE6D = 144,        /* 24 joints x 6 */
  JRR_DISC_PARAMS = 1840153,
  JRR_SHAPE_DISC_PARAMS = 171,
  JRR_SIL_SIZE = 224       /* silhouette image size (square) of an engine without JRR_FLAG_SIL_256; see jrr_silhouette_forward */
};

/* engine flags */
enum {
  JRR_FLAG_POSE_DISC = 1,   /* allocate / run the pose-discriminator term (optimize.py:241-247) */
  JRR_FLAG_SHAPE_DISC = 2,  /* shape-discriminator term (optimize.py:244,249-250) */
  JRR_FLAG_KEEP_VERTS = 4,  /* reserve a (B,6890,3) vertex buffer for return_verts / J step */
  JRR_FLAG_FOLDED = 8,      /* reserve the folded-regressor tables (jrr_engine_set_folded) */
  JRR_FLAG_SILHOUETTE = 16, /* reserve the soft-silhouette buffers (needs JRR_FLAG_KEEP_VERTS and model faces): per pose the projected
                               vertices of the stand-alone API (110 KB), the covered-pixel list (200 KB at 224 x 224) and a pose-major
                               copy of the vertices for the fused rasteriser (83 KB) */
  JRR_FLAG_NO_MODEL = 32,   /* discriminator-only engine (model == NULL): the SMPL sections (~230 KB per pose) are not
                               part of the workspace; only JRR_FLAG_POSE_DISC / JRR_FLAG_SHAPE_DISC may accompany it */
  JRR_FLAG_SIL_256 = 64,    /* with JRR_FLAG_SILHOUETTE: 256 x 256 silhouettes (the reference constructor's default,
                               scripts/mesh_renderer.py:25; focal length 5000 / 256) instead of 224 x 224 (scripts/optimize.py:110):
                               every (B,224,224) below then reads (B,256,256) */
  JRR_FLAG_SIL_SIZE_MASK = 15 << 16, /* with JRR_FLAG_SILHOUETTE: JRR_FLAG_SIL_SIZE(size) below -- an explicit image size, any multiple of 32
                               up to 256 (Mesh_Renderer(image_size), scripts/mesh_renderer.py:25,34-38; focal length 5000 / size).  Sizes other
                               than 224 and 256 serve the stand-alone renderer (jrr_silhouette_forward / _backward / _pix_to_face); the
                               silhouette term INSIDE the loop (jrr_engine_set_silhouette) is built for 224 and 256, the sizes the reference
                               instantiates.  0 = 224, or 256 with JRR_FLAG_SIL_256 */
  JRR_FLAG_SUPPORT_TILES = 128,/* with JRR_FLAG_KEEP_VERTS: once jrr_j_support_info has reported that the regressor's support fits,
                               the iterations of jrr_refine_run* whose loss reads the JOINTS only (no silhouette term) run their three
                               skinning kernels on the 32-vertex tiles that hold a support entry -- every other tile multiplies
                               its vertices by a zero block of the regressor and receives a zero vertex adjoint: exact zeros in
                               the joints and in every gradient.  Same numbers as without the flag up to the order of the sums
                               over the tiles; until jrr_j_support_info is called (and after a jrr_engine_set_j_regressor from
                               outside) the iterations run all 216 tiles.  v_posed / vertices of the other tiles are NOT
                               produced by those iterations (jrr_find_joints_forward and jrr_smpl_vertices* always are dense). */
  JRR_FLAG_BLEND_BF16X3 = 256  /* SIDE MODE, not the reference's arithmetic (the reference computes in fp32 and so does every engine
                               without this flag): the all-tiles blend-basis adjoint (jrr_refine_run*, jrr_find_joints_backward, jrr_smpl_vertices_backward) runs as a split-bf16 product
                               -- operands taken as bf16 hi + lo, three bf16 matrix instructions per exact-fp32 eight, fp32
                               accumulation; relative error of the product ~ 3e-5.  Reserves 18.6 MB for the split basis.  Every
                               other kernel, and the support-tile iterations, are unchanged.  bench.py reports it as a separately
                               labelled block (`bf16x3_mode`); it is never the headline. */
};

/* row of the refined-pose table (jrr_pose_export): JRR_EXPORT_ROW floats per sample, offsets in floats.  Layout version 1. */
enum {
  JRR_EXPORT_LAYOUT_VERSION = 1,
  JRR_EXPORT_ROW = 240,        /* 960 bytes: every row of a 16-byte aligned table is 16-byte aligned */
  JRR_EXPORT_POSE = 0,         /* 72: axis-angle of the 24 joints, orient first (SMPL's `pose`) */
  JRR_EXPORT_POSE6D = 72,      /* 144: the 6-D values, copied unchanged */
  JRR_EXPORT_BETAS = 216,      /* 10 */
  JRR_EXPORT_CAM = 226,        /* 3 */
  JRR_EXPORT_MARKER = 229,     /* 1.0f in a written row, 0 in a row nobody wrote */
  JRR_EXPORT_EXTRA = 230,      /* 10: the caller's per-sample values, zeros beyond n_extra */
  JRR_EXPORT_MAX_EXTRA = 10,
  JRR_EXPORT_STATUS_INDEX = 1, /* status bit 0: an index outside [0, n_rows); that row is not written */
  JRR_EXPORT_STATUS_TWICE = 2  /* status bit 1: the target row's marker was already set (a sample exported twice); overwritten */
};

/* jrr_pose_smooth / jrr_pose_jitter: the time-axis filter over the refined-pose table. */
enum {
  JRR_SMOOTH_MAX_RADIUS = 16,       /* the window is 2 radius + 1 positions; weights has radius + 1 entries */
  JRR_SMOOTH_TILE = 32,             /* positions per workgroup (a result never depends on where its position falls in a tile) */
  JRR_SMOOTH_MAX_POSITIONS = 1 << 30,
  JRR_SMOOTH_STATUS_INDEX = 1,      /* status bit 0: an entry of order outside [0, n_rows); that position is skipped */
  JRR_SMOOTH_STATUS_MARKER = 2      /* status bit 1: a listed row whose marker is not 1.0f; that position is skipped */
};

/* jrr_view_relrot_accumulate / jrr_view_fuse: the camera views of one instant, over the refined-pose table. */
enum {
  JRR_FUSE_MAX_VIEWS = 8,           /* members of one group (one scene and frame); a member lies within 7 positions of every other */
  JRR_FUSE_TILE = 32,               /* positions per workgroup (a result never depends on where its position falls in a tile) */
  JRR_FUSE_ACC_ROW = 12,            /* int64 per pair: count, the upper triangle of q q^T (ww wx wy wz xx xy xz yy yz zz) in units of 2^-24, one spare */
  JRR_FUSE_STATUS_INDEX = 1,        /* status bit 0: an entry of order outside [0, n_rows) */
  JRR_FUSE_STATUS_MARKER = 2,       /* status bit 1: a listed row whose marker is not 1.0f */
  JRR_FUSE_STATUS_WIDE = 4,         /* status bit 2: the position 8 places before or behind carries the same group id: the group continues
                                       beyond the 7 positions the kernels look at on either side */
  JRR_FUSE_STATUS_PAIR = 8          /* status bit 3: a pair id >= n_pairs (or a ref_pair entry outside [0, n_pairs)) */
};

/* row of the evaluation-report table (jrr_eval_accumulate): JRR_EVAL_ACC_ROW int64 per group, offsets in int64, then a trailer of
 * JRR_EVAL_ACC_TRAILER int64 behind the last row.  Layout version 1. */
enum {
  JRR_EVAL_ACC_LAYOUT_VERSION = 1,
  JRR_EVAL_ACC_ROW = 338,
  JRR_EVAL_ACC_COUNT = 0,       /* poses counted */
  JRR_EVAL_ACC_BAD = 1,         /* poses of this group left out: one of their 34 values fails e < 1.0e3f (NaN, inf, absurd) */
  JRR_EVAL_ACC_SUM = 2,         /* 17: sum over the poses of rn(err_j * 2^24), per joint (units of 2^-24 m) */
  JRR_EVAL_ACC_SUM_PA = 19,     /* 17: the same for err_pa_j */
  JRR_EVAL_ACC_HIST = 36,       /* 151: histogram of err_j over all 17 joints, bin min((int)floorf(e * 1000.f), 150) */
  JRR_EVAL_ACC_HIST_PA = 187,   /* 151: the same for err_pa_j */
  JRR_EVAL_ACC_BINS = 151,      /* 1-mm bins 0 .. 149, bin 150 = everything >= 150 mm */
  JRR_EVAL_ACC_TRAILER = 2,
  JRR_EVAL_ACC_TRAILER_IGNORED = 0,    /* poses with group < 0 (ignored on purpose) */
  JRR_EVAL_ACC_TRAILER_BAD_GROUP = 1,  /* poses with group >= n_groups (skipped; the caller treats non-zero as an error) */
  JRR_EVAL_ACC_MAX_GROUPS = 1024,
  JRR_REGRESS_MAX_REG = 4       /* regressors one jrr_regress_joints call applies to one read of the vertices */
};

/* row of the regressor report's table (jrr_regressor_shift_accumulate): JRR_SHIFT_ACC_ROW int64 per group, offsets in int64, then a
 * trailer of JRR_SHIFT_ACC_TRAILER int64 behind the last row, the trailer of the evaluation table.  Layout version 1.
 * Fixed point: a length c in metres is q = llrintf(c * 2^24) (the scaling is exact, one rounding to an integer).
 * Overflow, at the cap |c| < 4 m and 1e8 < 2^26.6 poses in one word: |q| < 2^26, so a sum of q stays below 2^52.6; a product
 * q_i * q_j is below 2^52, shifted by 16 below 2^36, summed below 2^62.6; |d| < 4 sqrt(3) (1 + 2^-20) < 2^2.8 m gives sums below
 * 2^53.4, the pelvis-relative length, at most twice that, below 2^54.4.  Counts and bins are at most the number of poses.       */
enum {
  JRR_SHIFT_ACC_LAYOUT_VERSION = 1,
  JRR_SHIFT_ACC_ROW = 1277,
  JRR_SHIFT_ACC_COUNT = 0,      /* poses counted */
  JRR_SHIFT_ACC_BAD = 1,        /* poses of this group left out (non-finite input, no body frame, a component at or beyond the cap) */
  JRR_SHIFT_ACC_SUM = 2,        /* [17][3]: sum of q over the poses, body-frame x, y, z (units of 2^-24 m) */
  JRR_SHIFT_ACC_MOM = 53,       /* [17][6]: sum of (q_i * q_j) >> 16, arithmetic shift of the int64 product, (i,j) = xx, xy, xz, yy, yz, zz
                                   (units of 2^-32 m^2) */
  JRR_SHIFT_ACC_ABS = 155,      /* [17]: sum of llrintf(|d| * 2^24) */
  JRR_SHIFT_ACC_ABS_REL = 172,  /* [17]: sum of llrintf(|d - d[Pelvis]| * 2^24) */
  JRR_SHIFT_ACC_HIST = 189,     /* [17][64]: histogram of |d|, bin min(63, (int)floorf(|d| * 500.0f)) */
  JRR_SHIFT_ACC_BINS = 64,      /* 2-mm bins 0 .. 62, bin 63 = everything >= 126 mm */
  JRR_SHIFT_ACC_TRAILER = 2,    /* JRR_EVAL_ACC_TRAILER_IGNORED, JRR_EVAL_ACC_TRAILER_BAD_GROUP */
  JRR_DISCS_MAX_SETS = 8,       /* jrr_draw_discs */
  JRR_DISCS_MAX_POINTS = 256
};

/* jrr_point_mesh_depth / jrr_depth_accumulate: the depth of points below a mesh surface, and the row of its table: JRR_DEPTH_ACC_ROW
 * int64 per group, offsets in int64, then the trailer of the evaluation table behind the last row.  Layout version 1.
 * Overflow: a depth below the cap 1.0e3f gives |llrintf(depth * 2^24)| < 2^34, so a sum stays below 2^63 for 5e8 poses in one word.
 * Counts and bins are at most the number of poses. */
enum {
  JRR_DEPTH_ACC_LAYOUT_VERSION = 1,
  JRR_DEPTH_MAX_POINTS = 64,        /* points per pose of one call: one lane of a wave each */
  JRR_DEPTH_MAX_VERTS = 8192,       /* vertices per pose: 96 KiB of the 160 KiB of LDS, beside the reduction scratch */
  JRR_DEPTH_STATUS_INDEX = 1,       /* status bit 0: a face with an index outside [0, n_verts); that face is skipped */
  JRR_DEPTH_ACC_ROW = 4290,
  JRR_DEPTH_ACC_COUNT = 0,          /* poses counted */
  JRR_DEPTH_ACC_BAD = 1,            /* poses of this group left out: one of their 2 n_points values is non-finite, or a dist fails d < 1.0e3f */
  JRR_DEPTH_ACC_OUTSIDE = 2,        /* [64]: poses whose point k is outside: !(fabsf(wind) > 0.5f) */
  JRR_DEPTH_ACC_UNSURE = 66,        /* [64]: poses with fabsf(|wind| - rintf(|wind|)) > 0.1f: the surface is not closed around point k, or k lies on it */
  JRR_DEPTH_ACC_SUM = 130,          /* [64]: sum of llrintf(depth * 2^24), depth = inside ? dist : -dist (units of 2^-24 m) */
  JRR_DEPTH_ACC_HIST = 194,         /* [64][64]: histogram of depth, bin max(0, min(63, (int)floorf((depth + 0.064f) * 250.0f))) */
  JRR_DEPTH_ACC_BINS = 64,          /* 4-mm bins over [-64, +192) mm; bin 0 also holds everything below, bin 63 everything above */
  JRR_DEPTH_ACC_TRAILER = 2         /* JRR_EVAL_ACC_TRAILER_IGNORED, JRR_EVAL_ACC_TRAILER_BAD_GROUP */
};

/* jrr_mesh_winding / jrr_penetration_accumulate: the winding number of a mesh around many points per pose, and the row of the
 * self-penetration table: JRR_PEN_ACC_ROW int64 per group, offsets in int64, then the trailer of the evaluation table behind the last
 * row.  Layout version 1.  Every word is a count: at most poses * vertices. */
enum {
  JRR_PEN_ACC_LAYOUT_VERSION = 1,
  JRR_WINDING_MAX_POINTS = 65536,   /* points per pose of one call; vertices per pose of jrr_penetration_accumulate */
  JRR_PEN_ACC_ROW = 55,
  JRR_PEN_ACC_COUNT = 0,            /* poses counted */
  JRR_PEN_ACC_BAD = 1,              /* poses of this group with a non-finite wind value; such a pose adds nothing else */
  JRR_PEN_ACC_POSES_PEN = 2,        /* poses with n_pen >= 1 */
  JRR_PEN_ACC_POSES_PEN8 = 3,       /* poses with n_pen >= 8: a few vertices can be mesh noise */
  JRR_PEN_ACC_SUM_PEN = 4,          /* sum of n_pen */
  JRR_PEN_ACC_SUM_THIN = 5,         /* sum of n_thin */
  JRR_PEN_ACC_SUM_UNSURE = 6,       /* sum of n_unsure */
  JRR_PEN_ACC_HIST = 7,             /* [16]: histogram of n_pen per pose, bin min(15, number of bits of n_pen): 0, 1, 2-3, 4-7, 8-15, ... */
  JRR_PEN_ACC_BINS = 16,
  JRR_PEN_ACC_PART = 23,            /* [32]: penetrating vertices by part[v]; a label outside [0, 32) goes to word 31, NULL parts to word 0 */
  JRR_PEN_ACC_PARTS = 32,
  JRR_PEN_ACC_TRAILER = 2           /* JRR_EVAL_ACC_TRAILER_IGNORED, JRR_EVAL_ACC_TRAILER_BAD_GROUP */
};

/* jrr_accel_error: the acceleration error along each video sequence, and the row of its table: JRR_ACCEL_ACC_ROW int64 per group,
 * offsets in int64, then the trailer of the evaluation table behind the last row.  Layout version 1.
 * Overflow: a value below the cap 1.0e3f gives llrintf(v * 2^24) < 2^34, so a sum stays below 2^63 for 5e8 triples in one word. */
enum {
  JRR_ACCEL_ACC_LAYOUT_VERSION = 1,
  JRR_ACCEL_TILE = 32,              /* positions per workgroup (a result never depends on where its position falls in a tile) */
  JRR_ACCEL_STATUS_INDEX = 1,       /* status bit 0: an entry of order outside [0, n_rows); that position is absent */
  JRR_ACCEL_ACC_ROW = 205,
  JRR_ACCEL_ACC_COUNT = 0,          /* triples scored */
  JRR_ACCEL_ACC_BAD = 1,            /* triples of this group left out: one of their 51 values e_j, s_j, g_j fails v < 1.0e3f (NaN, inf, absurd) */
  JRR_ACCEL_ACC_NO_TRIPLE = 2,      /* positions of this group without a triple */
  JRR_ACCEL_ACC_SUM_ERR = 3,        /* 17: sum over the triples of llrintf(e_j * 2^24), per joint (units of 2^-24 m per sampled frame^2) */
  JRR_ACCEL_ACC_SUM_PRED = 20,      /* 17: the same for s_j = |a_pred| */
  JRR_ACCEL_ACC_SUM_GT = 37,        /* 17: the same for g_j = |a_gt| */
  JRR_ACCEL_ACC_HIST = 54,          /* 151: histogram of e_j over all 17 joints, bin min((int)floorf(e * 1000.f), 150): the bins of JRR_EVAL_ACC_HIST */
  JRR_ACCEL_ACC_BINS = 151,
  JRR_ACCEL_ACC_TRAILER = 2         /* JRR_EVAL_ACC_TRAILER_IGNORED, JRR_EVAL_ACC_TRAILER_BAD_GROUP */
};

/* jrr_vertex_error: the per-vertex error of meshes, and the row of its group table: JRR_PVE_ACC_ROW int64 per group, offsets in
 * int64, then the trailer of the evaluation table behind the last row.  Layout version 1.
 * Overflow: a value below the cap 1.0e3f gives llrintf(v * 2^24) < 2^34, so a sum stays below 2^63 for 5e8 poses in one word. */
enum {
  JRR_PVE_ACC_LAYOUT_VERSION = 1,
  JRR_PVE_MAX_VERTS = 65536,        /* 1 <= n_verts <= 65536 */
  JRR_PVE_MAX_PARTS = 32,           /* 1 <= n_parts <= 32 */
  JRR_PVE_ACC_ROW = 370,
  JRR_PVE_ACC_COUNT = 0,            /* poses counted */
  JRR_PVE_ACC_BAD = 1,              /* poses of this group left out: pve or pa_pve is NaN */
  JRR_PVE_ACC_SUM = 2,              /* sum over the poses of llrintf(pve * 2^24) (units of 2^-24 m) */
  JRR_PVE_ACC_SUM_PA = 3,           /* the same for pa_pve */
  JRR_PVE_ACC_HIST = 4,             /* 151: histogram of the PER-POSE pve, bin min((int)floorf(pve * 1000.f), 150): the bins of JRR_EVAL_ACC_HIST */
  JRR_PVE_ACC_HIST_PA = 155,        /* 151: the same for pa_pve */
  JRR_PVE_ACC_PART = 306,           /* 32: sum over the poses of llrintf(m_p * 2^24), m_p the pose's mean plain error over part p */
  JRR_PVE_ACC_PART_PA = 338,        /* 32: the same for the aligned error */
  JRR_PVE_ACC_BINS = 151,
  JRR_PVE_ACC_TRAILER = 2           /* JRR_EVAL_ACC_TRAILER_IGNORED, JRR_EVAL_ACC_TRAILER_BAD_GROUP */
};

/* jrr_bone_error / jrr_bone_accumulate: bone length and direction errors of the 17-joint skeleton.  The per-pose values are ONE
 * packed (batch, JRR_BONE_VALS) fp32 array, offsets in floats; bone b = 1 .. 16 sits at index b - 1 of its block of 16, joint j at
 * index j of its block of 17.  The table: JRR_BONE_ACC_ROW int64 per group, offsets in int64, then the trailer of the evaluation table
 * behind the last row.  Layout version 1.
 * Overflow: a value below the cap 1.0e3f gives llrintf(v * 2^24) < 2^34, so a SUM word stays below 2^63 for 5e8 poses.  A length
 * below 1.0e3f m gives q = llrintf(len * 65536.f) < 2^26 and q * q < 2^52: a SUM_SQ word holds more than 10^3 poses AT the cap (2^11
 * of them), and 2^29 poses of bones shorter than 2 m (q < 2^17, q * q < 2^34). */
enum {
  JRR_BONE_ACC_LAYOUT_VERSION = 1,
  JRR_BONE_BONES = 16,              /* bone b joins joint b to its parent, b = 1 .. 16 */
  JRR_BONE_PAIRS = 6,               /* left / right pairs of bones */
  JRR_BONE_VALS = 98,               /* floats per pose: 4 x 16 + 2 x 17 */
  JRR_BONE_LEN_PRED = 0,            /* 16: len_pred_b, metres */
  JRR_BONE_LEN_GT = 16,             /* 16: len_gt_b, metres */
  JRR_BONE_ANG = 32,                /* 16: ang_b, radians */
  JRR_BONE_ANG_PA = 48,             /* 16: ang_pa_b, radians */
  JRR_BONE_ERR_DIR = 64,            /* 17: e_dir_j, metres */
  JRR_BONE_ERR_LEN = 81,            /* 17: e_len_j, metres */
  JRR_BONE_ACC_ROW = 192,
  JRR_BONE_ACC_COUNT = 0,           /* poses counted */
  JRR_BONE_ACC_BAD = 1,             /* poses of this group left out: one of their 98 values fails v < 1.0e3f (NaN, inf, absurd) */
  JRR_BONE_ACC_SUM_LEN_PRED = 2,    /* 16: sum over the poses of llrintf(len_pred_b * 2^24), per bone (units of 2^-24 m) */
  JRR_BONE_ACC_SUM_LEN_GT = 18,     /* 16: the same for len_gt_b */
  JRR_BONE_ACC_SUM_ABS_DLEN = 34,   /* 16: the same for fabsf(len_pred_b - len_gt_b) */
  JRR_BONE_ACC_SUM_ANG = 50,        /* 16: the same for ang_b (units of 2^-24 rad) */
  JRR_BONE_ACC_SUM_ANG_PA = 66,     /* 16: the same for ang_pa_b */
  JRR_BONE_ACC_SUM_SQ_PRED = 82,    /* 16: sum over the poses of q * q in int64, q = llrintf(len_pred_b * 65536.f) (units of 2^-32 m^2) */
  JRR_BONE_ACC_SUM_SQ_GT = 98,      /* 16: the same for len_gt_b */
  JRR_BONE_ACC_SUM_Q_PRED = 114,    /* 16: sum over the poses of that q itself (units of 2^-16 m): n SUM_SQ - SUM_Q^2 is n^2 x the variance, exactly */
  JRR_BONE_ACC_SUM_Q_GT = 130,      /* 16: the same for len_gt_b */
  JRR_BONE_ACC_SUM_ERR_DIR = 146,   /* 17: sum over the poses of llrintf(e_dir_j * 2^24), per joint */
  JRR_BONE_ACC_SUM_ERR_LEN = 163,   /* 17: the same for e_len_j */
  JRR_BONE_ACC_SUM_ASYM_PRED = 180, /* 6: sum over the poses of llrintf(fabsf(len_pred_left - len_pred_right) * 2^24), per pair */
  JRR_BONE_ACC_SUM_ASYM_GT = 186,   /* 6: the same for len_gt */
  JRR_BONE_ACC_TRAILER = 2          /* JRR_EVAL_ACC_TRAILER_IGNORED, JRR_EVAL_ACC_TRAILER_BAD_GROUP */
};

/* jrr_place_translation / jrr_place_accumulate (`--place_refined`): the camera-frame translation of a posed body under the real
 * intrinsics.  The status word of a pose, and the table: JRR_PLACE_ACC_ROW int64 per group, offsets in int64, then the trailer of the
 * evaluation table behind the last row.  Layout version 1.
 * Overflow: a pixel distance below the cap 1.0e3f gives llrintf(e * 2^24) < 2^34, so a SUM word stays below 2^63 for 5e8 poses. */
enum {
  JRR_PLACE_ACC_LAYOUT_VERSION = 1,
  JRR_PLACE_MAX_ITERS = 64,
  JRR_PLACE_FEW_OR_NONFINITE = 1,   /* bit 0: fewer than 2 taking-part joints, or a non-finite value among the pose's inputs */
  JRR_PLACE_LINEAR_PIVOT = 2,       /* bit 1: a pivot of the linear start's factorisation is not positive */
  JRR_PLACE_LINEAR_BEHIND = 4,      /* bit 2: the linear start leaves a taking-part joint at Z <= 0 */
  JRR_PLACE_STEP_PIVOT = 8,         /* bit 3: a pivot failed inside a Levenberg-Marquardt step (the step was rejected; the result is kept) */
  JRR_PLACE_BAD_BITS = 7,           /* a pose with one of bits 0 .. 2 holds NaN in trans and in both error rows */
  JRR_PLACE_ACC_ROW = 55,
  JRR_PLACE_ACC_COUNT = 0,          /* poses counted */
  JRR_PLACE_ACC_BAD = 1,            /* poses of this group left out: a status bit 0 .. 2, or a summed value that fails |v| < 1.0e3f */
  JRR_PLACE_ACC_STEP_PIVOT = 2,     /* counted poses with status bit 3 */
  JRR_PLACE_ACC_SUM_TZ = 3,         /* sum over the counted poses of llrintf((float)trans_z * 2^24) (units of 2^-24 m) */
  JRR_PLACE_ACC_JOINTS = 4,         /* 17: counted poses in which joint j takes part */
  JRR_PLACE_ACC_SUM_ERR_LIN = 21,   /* 17: sum over those of llrintf(err_lin_j * 2^24) (units of 2^-24 px) */
  JRR_PLACE_ACC_SUM_ERR = 38,       /* 17: the same for err_j */
  JRR_PLACE_ACC_TRAILER = 2         /* JRR_EVAL_ACC_TRAILER_IGNORED, JRR_EVAL_ACC_TRAILER_BAD_GROUP */
};

/* jrr_point_visibility / jrr_visibility_accumulate (`--visible_refined`): what the real camera sees of a placed body.  The bits of a
 * query's code, and the table: JRR_VIS_ACC_ROW int64 per group, offsets in int64, then the trailer of the evaluation table behind the
 * last row.  Layout version 1.
 * Overflow: an error below the cap 1.0e5f mm gives llrintf(e * 2^24) < 2^41, so a SUM_ERR word stays below 2^63 for 4e6 poses. */
enum {
  JRR_VIS_ACC_LAYOUT_VERSION = 1,
  JRR_VIS_MAX_POINTS = 65536,       /* queries per pose of one call; vertices per pose of jrr_visibility_accumulate */
  JRR_VIS_JOINTS = 17,
  JRR_VIS_OCCLUDED = 1,             /* code bit 0: at least min_crossings faces cross the ray in front of the query */
  JRR_VIS_OUTSIDE = 2,              /* code bit 1: the pixel lies outside the window */
  JRR_VIS_INVALID = 4,              /* code bit 2: depth <= 0 or a non-finite coordinate; bits 0 and 1 are then clear */
  JRR_VIS_ACC_ROW = 154,
  JRR_VIS_ACC_COUNT = 0,            /* poses counted */
  JRR_VIS_ACC_BAD = 1,              /* poses of this group left out whole (see jrr_visibility_accumulate) */
  JRR_VIS_ACC_SUM_VERT_SEEN = 2,    /* vertices of the counted poses with code 0 */
  JRR_VIS_ACC_SUM_VERT_OCCLUDED = 3,/* ... with bit 0 */
  JRR_VIS_ACC_SUM_VERT_OUTSIDE = 4, /* ... with bit 1 (a vertex with both bits counts in both words) */
  JRR_VIS_ACC_J_SEEN = 5,           /* 17: counted poses in which joint j has code 0 */
  JRR_VIS_ACC_J_OCCLUDED = 22,      /* 17: ... bit 0 set and bit 1 clear */
  JRR_VIS_ACC_J_OUTSIDE = 39,       /* 17: ... bit 1 set */
  JRR_VIS_ACC_SUM_ERR_SEEN = 56,    /* 17: sum over the poses of J_SEEN of llrintf(err_j * 2^24) (units of 2^-24 mm) */
  JRR_VIS_ACC_SUM_ERR_OCCLUDED = 73,/* 17: the same over the poses of J_OCCLUDED */
  JRR_VIS_ACC_PART_SEEN = 90,       /* [32]: vertices with code 0 by part[v]; a label outside [0, 32) goes to word 31, NULL parts to word 0 */
  JRR_VIS_ACC_PART_ALL = 122,       /* [32]: all vertices of the counted poses by part[v] */
  JRR_VIS_ACC_PARTS = 32,
  JRR_VIS_ACC_TRAILER = 2           /* JRR_EVAL_ACC_TRAILER_IGNORED, JRR_EVAL_ACC_TRAILER_BAD_GROUP */
};

/* The paired bootstrap of the evaluation report (`--eval_ci`): jrr_paired_units fills two int64 tables, jrr_bootstrap_sums resamples
 * the first.  Layout version 1.
 *   units  [n_units][JRR_BOOT_UNIT_ROW]: per resampling unit (a video sequence, or a frame) the sums over its counted poses.
 *   wins   [n_groups][JRR_BOOT_WINS_ROW] + JRR_BOOT_WINS_TRAILER words behind the last row.
 * Overflow: a counted pose has 17 values below 1.0e3f per column, so its sum is below 17 * 10^3 * 2^24 < 2^39.  A replicate adds
 * count_s unit rows: BEFORE the launch the host computes, in unbounded integers, (largest count_s) x (largest word of the unit table)
 * and refuses when it reaches 2^62 -- nothing overflows silently. */
enum {
  JRR_BOOT_LAYOUT_VERSION = 1,
  JRR_BOOT_UNIT_ROW = 5,
  JRR_BOOT_UNIT_BEFORE = 0,         /* sum over the unit's poses of sum_j rn(err_j * 2^24), initial regressor (units of 2^-24 m) */
  JRR_BOOT_UNIT_BEFORE_PA = 1,      /* the same for err_pa_j */
  JRR_BOOT_UNIT_AFTER = 2,          /* retrained regressor */
  JRR_BOOT_UNIT_AFTER_PA = 3,
  JRR_BOOT_UNIT_COUNT = 4,          /* poses counted */
  JRR_BOOT_WINS_ROW = 8,
  JRR_BOOT_WINS_COUNT = 0,          /* poses counted */
  JRR_BOOT_WINS_BAD = 1,            /* poses of this group left out for BOTH regressors: one of their 68 values fails e < 1.0e3f */
  JRR_BOOT_WINS_BETTER = 2,         /* counted poses whose AFTER sum is smaller than their BEFORE sum (integer comparison) */
  JRR_BOOT_WINS_WORSE = 3,          /* ... larger */
  JRR_BOOT_WINS_TIE = 4,            /* ... equal */
  JRR_BOOT_WINS_BETTER_PA = 5,      /* the same three for the aligned sums */
  JRR_BOOT_WINS_WORSE_PA = 6,
  JRR_BOOT_WINS_TIE_PA = 7,
  JRR_BOOT_WINS_TRAILER = 3,
  JRR_BOOT_WINS_TRAILER_IGNORED = 0,    /* poses with group < 0 (ignored on purpose) */
  JRR_BOOT_WINS_TRAILER_BAD_GROUP = 1,  /* poses with group >= n_groups (the caller treats non-zero as an error) */
  JRR_BOOT_WINS_TRAILER_BAD_UNIT = 2,   /* poses with a unit outside [0, n_units) (likewise) */
  JRR_BOOT_MAX_SEGMENTS = 1025          /* all units + one segment per group (JRR_EVAL_ACC_MAX_GROUPS) */
};

#define JRR_FLAG_SIL_SIZE(size) ((((size) / 32) & 15) << 16)

typedef struct jrr_model jrr_model_t;   /* device-resident, re-laid-out SMPL constants */
typedef struct jrr_engine jrr_engine_t; /* per-batch plan: workspace carve-up + launch geometry */

const char* jrr_last_error(void);
int jrr_version(void);

/* ---- SMPL model ---------------------------------------------------------------------------
 * Replaces SMPL("SPIN/data/smpl", batch_size=1).to(device) (scripts/optimize.py:96-99;
 * wrapper scripts/smpl.py:61-85).  Host arrays in smplx layout:
 *   v_template (6890,3)  shapedirs (6890,3,10)  posedirs (207,20670)
 *   J_regressor (24,6890)  lbs_weights (6890,24)  parents (24)
 * Uploads tile-major copies of the blend basis / skinning weights and the folded rest-joint
 * regressor (J_template, J_shapedirs).  Synchronous.                                         */
int jrr_model_create(const float* v_template_host, const float* shapedirs_host,
                     const float* posedirs_host, const float* J_regressor_host,
                     const float* lbs_weights_host, const int32_t* parents_host,
                     jrr_model_t** out);
void jrr_model_destroy(jrr_model_t* m);
/* The same with the model's device memory owned by the CALLER (the caller owns every buffer):
 * buffer_dev = jrr_model_bytes() bytes, 256-byte aligned, it must outlive the model; NULL = the library allocates its own
 * (what jrr_model_create does).  The buffer also holds the face lists of jrr_model_set_faces.                              */
size_t jrr_model_bytes(void);
int jrr_model_create_in(const float* v_template_host, const float* shapedirs_host, const float* posedirs_host,
                        const float* J_regressor_host, const float* lbs_weights_host, const int32_t* parents_host,
                        void* buffer_dev, size_t buffer_bytes, jrr_model_t** out);
/* ... with a HINT for the internal vertex order: hint_vertices_host[n_hint] (file indices; duplicates ignored) are the vertices the
 * caller's H36M regressor will read -- the columns where it is positive.  They are stored first (ceil(n / 32) tiles instead of
 * up to one tile per vertex), which is what the iterations of JRR_FLAG_SUPPORT_TILES run; everything visible at the API keeps the
 * file's vertex order.  The hint is dropped (jrr_model_info out[29] = 0) when one of those tiles would see more than 16 joints.
 * A regressor with OTHER positive columns works as before, on more tiles.  No reference counterpart: the reference multiplies
 * all 6890 vertices by the regressor (scripts/utils.py:87-92).                                                              */
int jrr_model_create_hinted(const float* v_template_host, const float* shapedirs_host, const float* posedirs_host,
                            const float* J_regressor_host, const float* lbs_weights_host, const int32_t* parents_host,
                            const int32_t* hint_vertices_host, int n_hint, void* buffer_dev, size_t buffer_bytes, jrr_model_t** out);
/* What the LBS kernels will run for this body (measurement / diagnostics; the reference has no counterpart):
 * out[0] = joint slots per 32-vertex tile and pass of the joint-sparse kernels (8 or 12; 0 = the dense kernels),
 * out[1] = WIDE tiles (more joints than that: each runs a second pass -- it costs itself, not the model),
 * out[2] = most joints of any tile, out[3] = 1 when the vertices are stored in the library's own joint-sorted order
 * (invisible at the API), out[4 + k] = number of tiles with k joints, k = 0 .. 24, out[29] = vertices stored first on the
 * caller's hint (jrr_model_create_hinted; 0 = no hint or hint dropped).                                                  */
int jrr_model_info(const jrr_model_t* m, int32_t* out, int n);
/* triangle list of the mesh (SMPL `f`, 13776 x 3 int32; the reference reads it from data/body_model/smpl_uv.obj,
 * scripts/mesh_renderer.py:40-41); needed by the silhouette renderer only.  Synchronous.                  */
int jrr_model_set_faces(jrr_model_t* m, const int32_t* faces_host, int n_faces);

/* ---- engine -------------------------------------------------------------------------------
 * `batch` = poses on this device; `batch_norm` = divisor batch of the MSE means
 * (== batch single-GPU; == global batch under data parallelism so that a sharded run equals
 * the single-process run).  The caller owns `workspace_dev`: jrr_engine_workspace_bytes bytes,
 * 256-byte aligned and ZERO-FILLED at creation (padding rows / columns of several sections are operands of the matrix
 * kernels and are never written).
 * `model` may be NULL for an engine that serves the discriminators only (flags within
 * JRR_FLAG_POSE_DISC | JRR_FLAG_SHAPE_DISC): Discriminator / Shape_Discriminator modules need no body model. */
size_t jrr_engine_workspace_bytes(int batch, int flags);
int jrr_engine_create(const jrr_model_t* model, int batch, int batch_norm, void* workspace_dev,
                      size_t workspace_bytes, int flags, jrr_engine_t** out);
void jrr_engine_destroy(jrr_engine_t* e);
int jrr_engine_set_batch_norm(jrr_engine_t* e, int batch_norm);
/* Folded joint regression for jrr_refine_run (needs JRR_FLAG_FOLDED): the pose-independent contraction
 * H = sum_v Jn W D (1224 x 218) is rebuilt at every jrr_engine_set_j_regressor, and each iteration evaluates
 * joints = A . (H F) instead of skinning 6890 vertices -- the same function of (theta, beta, J) up to fp32
 * rounding, ~25x fewer FLOP, no vertices.  A separate mode with its own denominator; never the default.   */
int jrr_engine_set_folded(jrr_engine_t* e, int enabled, void* stream);
/* J*mask -> ReLU -> row-normalise (scripts/utils.py:87-92), into the engine's tile-major
 * copies.  J_dev: (17,6890) row-major raw parameter; mask_dev may be NULL.                   */
int jrr_engine_set_j_regressor(jrr_engine_t* e, const float* J_dev, const float* mask_dev, void* stream);

/* Pose-discriminator weights (scripts/discriminator.py:7-30) as ONE flat fp32 vector in
 * state_dict order: conv_operations.{0,2}.{weight,bias}, linears.{0..23}.{weight,bias},
 * linear_operations.{0,2,4}.{weight,bias} (1 840 153 floats).  Shape discriminator
 * (discriminator.py:57-68): shape_operations.{0,2,4}.{weight,bias} (171 floats).            */
int jrr_engine_set_pose_disc(jrr_engine_t* e, const float* params_dev, void* stream);
int jrr_engine_set_shape_disc(jrr_engine_t* e, const float* params_dev, void* stream);

/* ---- operator-level entry points (autograd.Function backends) ------------------------------ */

/* rot6d_to_rotmat, scripts/utils.py:190-204: x (n,6) -> R (n,3,3); and its adjoint.          */
int jrr_rot6d_forward(const float* x6d_dev, float* R_dev, int n, void* stream);
int jrr_rot6d_backward(const float* x6d_dev, const float* dR_dev, float* dx6d_dev, int n, void* stream);

/* ---- dataset images ------------------------------------------------
 * find_crop, scripts/data.py:220-271 (called twice per sample at :123-127): the square crop around a bounding box through the
 * similarity warp of scripts/perturbation_helper.py:185-210 with theta = 0, the sampling grid of scripts/sampling_helper.py:42-69
 * and grid_sample (bilinear, zero padding, align_corners=False), for a whole batch of uint8 frames in ONE launch.
 *   pixels_dev   uint8, interleaved RGB (H,W,3) rows; 16-byte aligned, pixels_bytes a non-zero multiple of 16
 *   desc_dev     [batch][8] int64 per sample {byte offset, row pitch in bytes, roi_y0, roi_x0, roi_h, roi_w, frame_H, frame_W}: the
 *                buffer holds the block [roi_y0, roi_y0 + roi_h) x [roi_x0, roi_x0 + roi_w) of a frame_H x frame_W frame (roi_w <= 1024;
 *                the whole frame is the block (0, 0, H, W)).  The caller hands over at least the rows and columns the crops read.
 *   bboxes_dev   [batch][4] (min_y, min_x, max_y, max_x) in the reference's 1000-unit frame convention whatever the frame's size
 *   mean_dev / std_dev   [3] each or both NULL: (x - mean) / std per channel on the size0 crop (transforms.Normalize,
 *                scripts/optimize.py:141-142,164)
 *   size0 / out0_dev, size1 / out1_dev   crop sizes (multiples of 4, at most 256; size1 = 0: one crop) and their outputs
 *                (batch,3,size,size) float32 in [0, 1]: uint8 / 255 (scripts/data.py:113) interpolated
 *   status_dev   one int32 the CALLER zeroes and reads when it next synchronises.  Bit 0: a bilinear tap of non-zero weight inside the
 *                frame lies outside the sample's block (nothing is read there; the value is wrong); bit 1: a descriptor does not fit
 *                the pixel buffer (that sample reads nothing).  Never cleared by the library.
 * A bounding box of zero size gives non-finite sampling positions and an all-zero crop (scripts/sampling_helper.py:36-38).    */
int jrr_image_crop(const uint8_t* pixels_dev, size_t pixels_bytes, const int64_t* desc_dev, const float* bboxes_dev, int batch,
                   const float* mean_dev, const float* std_dev, int size0, float* out0_dev, int size1, float* out1_dev,
                   int32_t* status_dev, void* stream);
/* mask_rcnn of scripts/data.py:117-121,130-132: masks_dev uint8 (batch,h,w) -> out_dev float32 (batch,1,h,w) = mask / 255 with
 * the 2 x 2 corner [:2, :2] zeroed, valid_dev int32 (batch) = (mask[0, 0] != 0) read BEFORE the corner is zeroed.             */
int jrr_mask_prepare(const uint8_t* masks_dev, int batch, int h, int w, float* out_dev, int32_t* valid_dev, void* stream);

/* ---- fit report: how well a rendered silhouette covers its mask, and a picture of it -----------------------------------
 * viz() of scripts/optimize.py:35-48 as the reference calls it around its inner loop (:204-218 before, :268-274 after the 100
 * iterations): r = render > thr_render (0.5 there), m = mask_rcnn > thr_mask (0.8), both STRICT and compared in fp32 as torch.where
 * on float32 tensors does (mask byte 204 / 255 = 0.800000012 is not above float32(0.8); byte 205 is); NaN compares false.
 *   alpha_dev, mask_dev   (batch,h,w) float32, 16-byte aligned, h * w a multiple of 4 (every pose is read as float4)
 *   counts_dev            [batch][4] int32 {r & m, r | m, r, m} summed over the pose's pixels; zeroed by the call itself.  Integer sums:
 *                         bit-reproducible.  IoU = counts[0] / counts[1] (both empty: the silhouettes agree).                          */
int jrr_silhouette_compare(const float* alpha_dev, const float* mask_dev, int batch, int h, int w, float thr_render, float thr_mask,
                           int32_t* counts_dev, void* stream);
/* The picture: rgb_dev (batch,size,size,3) uint8, interleaved (what a PNG encoder takes); size a multiple of 4, at most 256.
 *   image_dev     (batch,3,size,size) float32 or NULL (background 0); mean_dev / std_dev [3] each or both NULL: the image is the
 *                 normalised SPIN crop (scripts/optimize.py:141-142,164) and x * std + mean undoes it (product rounded, then the sum)
 *   joints2d_dev  (n_sets,batch,17,2) in the crop's pixel frame, 0 <= n_sets <= 3 (NULL with 0)
 * Arithmetic, every step rounded once in fp32, so that a host restatement reproduces every byte:
 *   1. background byte = (uint8) floorf(fminf(fmaxf(x, 0), 1) * 255.0f + 0.5f)
 *   2. where r or m, per channel out = (bg + tint + 1) >> 1 with tint (255,0,0) render only, (0,0,255) mask only, (0,255,0) both
 *      (the reference shows render + mask == 1, scripts/optimize.py:47-48); elsewhere out = bg
 *   3. joint discs last, a later set over an earlier one: set 0 (0,255,0) -- the target joints, green in the reference's scatter
 *      (:63-64) --, set 1 (255,255,0), set 2 (255,0,255).  Pixel (x, y) has its centre at the integer coordinate (imshow); it is
 *      inside a disc iff dx * dx + dy * dy <= radius * radius with dx = (float)x - jx.  A joint with a non-finite coordinate draws
 *      nothing; discs are clipped to the image.                                                                                    */
int jrr_fit_overlay(const float* alpha_dev, const float* mask_dev, const float* image_dev, const float* mean_dev, const float* std_dev,
                    const float* joints2d_dev, int n_sets, int batch, int size, float thr_render, float thr_mask, float radius,
                    uint8_t* rgb_dev, void* stream);

/* ---- fit report: shaded views of the fitted mesh (`--fit_report_mesh`) ------------------------------------------------------
 * What the reference had pytorch3d for (scripts/mesh_renderer.py:23-79 builds the silhouette renderer only; a shaded view is what a
 * person checks before trusting a fit).  Neither operator takes an engine or a body model; vertices and faces are in the API (file)
 * vertex order; n_verts and n_faces are general.  Every operation below is rounded once in fp32, in the order written; no product is
 * fused into a sum: the results are functions of the inputs alone (no float atomics) and a host restatement can follow them.  Every index
 * read from device memory is checked against its array before use: nothing is read outside the arrays whatever the data.
 *
 * jrr_vertex_normals: pytorch3d's Meshes.verts_normals_packed.
 *   verts_dev (batch,n_verts,3), faces_dev (n_faces,3) int32, normals_dev (batch,n_verts,3)
 *   adj_offset_dev [n_verts + 1], adj_face_dev [3 * n_faces] int32: the faces of vertex v are adj_face[adj_offset[v] .. adj_offset[v + 1]),
 *   in ascending face index (CSR; a vertex may have any number of them).
 *   Per (pose, vertex): s = 0; for every face f of the list, in the list's order, with p0, p1, p2 its vertices, e1 = p1 - p0, e2 = p2 - p0:
 *     s += (e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x)      (area-weighted: not normalised per face)
 *   len = sqrtf((sx * sx + sy * sy) + sz * sz), n = s / (len < 1e-6f ? 1e-6f : len) -- torch's clamp(min = 1e-6), which keeps a NaN.
 *   A vertex without faces gives exactly (0,0,0).  A non-finite vertex makes the normals of the vertices that share a face with it NaN,
 *   in its own pose, and nothing else.  A list entry or a vertex index outside its array is skipped.  */
int jrr_vertex_normals(const float* verts_dev, const int32_t* faces_dev, const int32_t* adj_offset_dev, const int32_t* adj_face_dev,
                       int batch, int n_verts, int n_faces, float* normals_dev, void* stream);
/* jrr_mesh_shade: the picture of the mesh behind a pix_to_face map (jrr_silhouette_pix_to_face): rgb_dev (batch,size,size,3) uint8,
 * interleaved; size a multiple of 4, at most 256.
 *   verts_dev, normals_dev (batch,n_verts,3); faces_dev (n_faces,3) int32; cam_dev (batch,3); pix_to_face_dev (batch,size,size) int32,
 *   16-byte aligned
 *   image_dev / mean_dev / std_dev   the background as in jrr_fit_overlay: (batch,3,size,size) float32 or NULL, x * std + mean (product
 *                 rounded, then the sum) when mean / std are given; without an image every pixel's x is `background`.  bg = fminf(fmaxf(x, 0), 1)
 *   colour_host, light_host [3]      base colour c in [0, 1] and the light direction l in view space, used as given (the caller normalises);
 *                 the headlight is (0, 0, -1)
 *   depth_dev (batch,size,size), normal_dev (batch,size,size,3)   nullable, 16-byte aligned
 *   status_dev    nullable; one int32 the CALLER zeroes and reads when it next synchronises, never cleared by the library
 * Per pixel (row i, column j) with face f = pix_to_face >= 0 and its vertices k = 0, 1, 2 (model-space position p_k, normal n_k):
 *   1. projection, as the rasteriser's k_sil_project: X = -2 x + cx, Y = -2 y + cy, Z_k = 2 z + cz, (u_k, v_k) = (F * X / Z_k, F * Y / Z_k)
 *      with F = 5000.0f / (float)size; pixel centre (px, py) = (1 - (float)(2 j + 1) / (float)size, 1 - (float)(2 i + 1) / (float)size)
 *   2. E(p; a, b) = (px - ax) * (by - ay) - (py - ay) * (bx - ax); area = E((u2,v2); 0, 1);
 *      w0 = E(p; 1, 2) / area, w1 = E(p; 2, 0) / area, w2 = E(p; 0, 1) / area          (no perspective correction: pytorch3d 0.3.0's default)
 *   3. pytorch3d's clip_barycentric_coordinates: w_k = fmaxf(w_k, 0), then w_k = w_k / fmaxf((w0 + w1) + w2, 1e-5f) -- a pixel whose centre
 *      lies just outside its face (the rasteriser's projection is compiled with other contraction choices) still gets a bounded answer
 *   4. depth = (w0 * Z_0 + w1 * Z_1) + w2 * Z_2
 *   5. m = (w0 * n_0 + w1 * n_1) + w2 * n_2 per component; view-space n = (-mx, -my, mz) / fmaxf(sqrtf((mx * mx + my * my) + mz * mz), 1e-6f)
 *   6. I = ambient + (1 - ambient) * |(nx * lx + ny * ly) + nz * lz|: TWO-SIDED -- a mesh whose faces wind inward (the synthetic body) is
 *      shaded like one that winds outward (the SMPL file)
 *   7. per channel byte = (uint8) floorf(fminf(fmaxf((opacity * c) * I + (1 - opacity) * bg, 0), 1) * 255.0f + 0.5f)
 * A pixel with f < 0: byte = floorf(bg * 255.0f + 0.5f), depth -1 (pytorch3d's zbuf convention), normal 0.  f >= n_faces, or a vertex index
 * of face f outside [0, n_verts): the same, and status bit 0.  A face with !(|area| > 1e-8f), or a non-finite u_k, v_k or Z_k: the same, and
 * status bit 1.                                                                                                                        */
enum { JRR_SHADE_STATUS_INDEX = 1, JRR_SHADE_STATUS_DEGENERATE = 2 };
int jrr_mesh_shade(const float* verts_dev, const float* normals_dev, const int32_t* faces_dev, const float* cam_dev,
                   const int32_t* pix_to_face_dev, const float* image_dev, const float* mean_dev, const float* std_dev, int batch, int n_verts,
                   int n_faces, int size, const float* colour_host, float opacity, float ambient, const float* light_host, float background,
                   uint8_t* rgb_dev, float* depth_dev, float* normal_dev, int32_t* status_dev, void* stream);

/* Axis-angle -> rotation matrix, smplx 0.1.26 lbs.batch_rodrigues: the pose2rot=True branch of the SMPL operator
 * (smplx.SMPL.forward default; the reference's wrapper inherits it, scripts/smpl.py:61-85, base class :7-9).
 * aa (n,3) -> R (n,3,3) with theta = |aa + 1e-8|, R = I + sin(theta) K + (1-cos(theta)) K^2; and its adjoint
 * dR (n,3,3) -> daa (n,3), finite at aa = 0.                                                               */
int jrr_rodrigues_forward(const float* aa_dev, float* R_dev, int n, void* stream);
int jrr_rodrigues_backward(const float* aa_dev, const float* dR_dev, float* daa_dev, int n, void* stream);

/* Rotation matrix -> axis-angle: R (n,3,3) row-major, assumed rotations -> aa (n,3).  Inverts jrr_rodrigues_forward up to that
 * kernel's own `+1e-8` quirk (its theta is |aa + 1e-8|).  Canonical form: the angle |aa| lies in [0, pi]; a rotation by exactly pi,
 * where aa and -aa denote the same matrix, gives the vector whose first non-zero component is positive (diag(-1,-1,1) -> (0,0,pi)).
 * The exact identity gives exactly 0.  No acos and no division by sin(theta): an unnormalised quaternion by Shepperd's choice
 * (the largest of tr, R00, R11, R22, ties in that order), then aa = (x,y,z) * 2 atan2(s, w) / s with s = |(x,y,z)| (a two-term
 * series when s <= 1e-4 w): fp32-accurate at every angle, pi included.  Non-finite input gives non-finite output for that
 * rotation only.  Not differentiable (no adjoint is provided).  No reference counterpart: the reference's (dead)
 * scripts/create_smpl_gt.py is the pseudo-ground-truth creator this serves.                                                  */
int jrr_rotmat_to_axis_angle(const float* R_dev, float* aa_dev, int n, void* stream);
/* The refined poses of one outer batch as per-sample records (`--save_refined`), ONE launch: per pose b the row
 *   [ axis-angle of rot6d_to_rotmat(x6d[b]) (72) | x6d[b] (144) | betas[b] (10) | cam[b] (3) | 1.0f | extra[b], zero-padded (10) ]
 * (JRR_EXPORT_* above) is written to row index_dev[b] of table_dev (n_rows, JRR_EXPORT_ROW), 16-byte aligned.  The axis-angle is
 * jrr_rotmat_to_axis_angle of the matrices the loop's own 6-D map gives (scripts/utils.py:190-204): canonical form as there --
 * angle in [0, pi], at pi the first non-zero component positive --, it inverts jrr_rodrigues_forward up to that kernel's own
 * `+1e-8` quirk.  Everything else is copied bit for bit.
 *   extra_dev    (batch,n_extra) or NULL (then n_extra values of zero), 0 <= n_extra <= JRR_EXPORT_MAX_EXTRA
 *   index_dev    (batch) int64
 *   status_dev   one int32 the CALLER zeroes and reads when it next synchronises, never cleared by the library: bit 0
 *                (JRR_EXPORT_STATUS_INDEX) an index outside [0, n_rows) -- that row is not written, nothing else is affected; bit 1
 *                (JRR_EXPORT_STATUS_TWICE) the target row's marker was already non-zero -- the row is overwritten.
 * The caller zero-fills the table once; rows nobody wrote keep marker 0.  Touches no engine.                                  */
int jrr_pose_export(const float* x6d_dev, const float* betas_dev, const float* cam_dev, const float* extra_dev, int n_extra,
                    const int64_t* index_dev, float* table_dev, int64_t n_rows, int32_t* status_dev, int batch, void* stream);

/* The refined poses of a table along the time axis (`--smooth_refined`).  table_dev (n_rows, JRR_EXPORT_ROW) is a table
 * jrr_pose_export wrote; it is only read.  order_dev (m) int32 lists table rows in time order and run_dev (m) int32 gives each
 * position's run of consecutive frames (the host forms both from the frame paths).  Position p's NEIGHBOURS are the offsets
 * k in [-radius, radius] with 0 <= p + k < m, run[p + k] == run[p] and position p + k not skipped (below).
 *   unit quaternion q of a joint of a row: R = rot6d_to_rotmat of the row's six values (scripts/utils.py:190-204, the loop's own map);
 *     Shepperd's unnormalised quaternion of R -- of tr, R00, R11, R22 the largest (ties in that order) selects
 *       (w,x,y,z) = (1+tr, R21-R12, R02-R20, R10-R01) | (R21-R12, 1+R00-R11-R22, R01+R10, R02+R20) | the two cyclic analogues,
 *     as in jrr_rotmat_to_axis_angle --; divided by its norm sqrt(w w + x x + y y + z z).  No canonical sign is chosen.
 *   jrr_pose_smooth, per position p and joint, with q_0 the centre's own quaternion and weights_dev[k] = (float)exp(-k k / (2 sigma^2))
 *   (the caller rounds them once; the kernel calls no exp):
 *     s = sum over the neighbours k, ascending from -radius, of weights[|k|] * (q_k . q_0 < 0 ? -q_k : q_k);
 *     s . q_0 >= weights[0] > 0, so the sum never degenerates;  q~ = s / |s|;
 *     x6d_out[p][joint] = the first two columns of R(q~) in the 6-D layout (x[0], x[2], x[4] column 0 =
 *       (1 - 2(yy + zz), 2(xy + wz), 2(xz - wy));  x[1], x[3], x[5] column 1 = (2(xy - wz), 1 - 2(xx + zz), 2(yz + wx)));
 *     delta_deg[p] = (sum over the 24 joints, in joint order, of 2 atan2(|e_xyz|, |e_w|) 180 / pi) / 24 with e = conj(q_0) (x) q~,
 *       conj(a) (x) b = (a.b,  a_w b_v - b_w a_v - a_v x b_v);
 *     betas_out[p], cam_out[p] = (sum_k weights[|k|] v_k) / (sum_k weights[|k|]) over the same neighbours in the same order, both
 *       sums starting from their first term.
 *   Every operation after rot6d_to_rotmat is rounded once, in the order written (no contraction).  With radius 0, or a run of
 *   length 1, betas_out and cam_out reproduce the row bit for bit and x6d_out holds the orthonormalised columns of the input.
 *   A non-finite row changes exactly the positions whose window holds it.
 *   jrr_pose_jitter, per position p whose neighbours p - 1 and p + 1 both exist: per joint d1 = conj(q_{p-1}) (x) q_p,
 *     d2 = conj(q_p) (x) q_{p+1}, e = conj(d1) (x) d2; jitter_deg[p] = the mean over the joints (summed in joint order) of the angle of
 *     e as above: degrees per sampled frame^2, zero for a constant angular velocity about a fixed axis.  NaN at every other position.
 *   begin, count   the positions [begin, begin + count) the call computes; the output arrays are indexed by position (m rows) and the
 *                  other rows are not touched.  A result depends on its window alone: not on m, the range or the launch's tiling.
 *   x6d_out_dev (m,24,6) 16-byte aligned, betas_out_dev (m,10), cam_out_dev (m,3), delta_deg_dev (m), jitter_deg_dev (m)
 *   status_dev     one int32 the CALLER zeroes and reads when it next synchronises: bit 0 (JRR_SMOOTH_STATUS_INDEX) an entry of order
 *                  outside [0, n_rows); bit 1 (JRR_SMOOTH_STATUS_MARKER) a listed row whose marker is not 1.0f.  Such a position is
 *                  skipped -- it is nobody's neighbour and its own outputs are NaN --; every other position is unaffected.
 * 0 <= radius <= JRR_SMOOTH_MAX_RADIUS.  Touches no engine.  No reference counterpart.                                          */
int jrr_pose_smooth(const float* table_dev, int64_t n_rows, const int32_t* order_dev, const int32_t* run_dev, int m,
                    const float* weights_dev, int radius, int begin, int count, float* x6d_out_dev, float* betas_out_dev,
                    float* cam_out_dev, float* delta_deg_dev, int32_t* status_dev, void* stream);
int jrr_pose_jitter(const float* table_dev, int64_t n_rows, const int32_t* order_dev, const int32_t* run_dev, int m, int begin, int count,
                    float* jitter_deg_dev, int32_t* status_dev, void* stream);

/* The refined poses of a table across the camera views of one instant (`--fuse_refined`).  table_dev as above, only read.  The host
 * forms three lists from the frame paths: order_dev (m) int32, the table rows sorted by (scene, frame, camera); group_dev (m) int32, the
 * (scene, frame) of each position, never decreasing, the members of a group contiguous; pair_dev (m) int32, the position's (scene,
 * camera) in [0, n_pairs) or -1 (no key, or a duplicate).  A position is VALID when its order entry lies in [0, n_rows), the row's marker
 * is 1.0f, its pair id is below n_pairs and neither position p - 8 nor p + 8 carries its group id; any other position raises its bit
 * of JRR_FUSE_STATUS_* in status_dev (one int32 the CALLER zeroes), is nobody's member, and its own outputs are NaN (floats) or 0
 * (counts); every other position is unaffected.  The MEMBERS of p's group: the valid positions within 7 places of p that carry its
 * group id, ascending -- at most JRR_FUSE_MAX_VIEWS.  Unit quaternion q of a joint of a row: as for jrr_pose_smooth.
 * a (x) b is the Hamilton product (w = aw bw - ax bx - ay by - az bz, x = aw bx + ax bw + ay bz - az by, y = aw by - ax bz + ay bw +
 * az bx, z = aw bz + ax by - ay bx + az bw, each summed left to right); conj(a) (x) b as for jrr_pose_smooth.  Every operation after
 * rot6d_to_rotmat is rounded once, in the order written.
 *   jrr_view_relrot_accumulate, per position p in [begin, begin + count) with c = pair[p] >= 0 and ref_pair_dev[c] != c (ref_pair_dev
 *   (n_pairs) int32: the pair of the scene's reference camera): the first member of p's group whose pair is ref_pair[c], if there is
 *   one, gives e = q_ref(joint 0) (x) conj(q_p(joint 0)), the quaternion of R_ref R_p^T;  acc[c][0] += 1 and
 *   acc[c][1 + t] += llrintf((e_i * e_j) * 2^24) for the ten pairs i <= j in the order ww wx wy wz xx xy xz yy yz zz (even in e: its sign
 *   is immaterial).  A non-finite e is not counted.  Integer atomics only: acc_dev (n_pairs, JRR_FUSE_ACC_ROW) int64, zeroed ONCE by the
 *   caller, is a function of the multiset of positions, whatever their order and the split into calls.
 *   jrr_view_fuse, per position p in [begin, begin + count) and joint j, with rel_dev (n_pairs, 4) float32 the rotations d_c (w,x,y,z)
 *   with R_ref ~ D_c R_c, all-zero = unknown (16-byte aligned):
 *     candidates  j >= 1: every member k, with q_k.   j = 0: the members with pair >= 0 and rel[pair] non-zero, with
 *                 q'_k = d_pair(k) (x) q_k.  If p itself is none, its six values are copied and delta_orient_deg[p] = NaN.
 *     anchor a    cos_half_max <= 0 (the plain mean): the first candidate, and every candidate is taken.  Otherwise the candidate of least
 *                 cost_k = sum over the candidates m != k, ascending, of (1 - |q_k . q_m|), a tie going to the lowest position; taken are
 *                 the candidates with |q_k . q_a| >= cos_half_max (the caller passes (float)cos(max_deg / 2)).
 *     s = sum over the taken k, ascending and starting from the first term, of (q_k . q_a < 0 ? -q_k : q_k);  f = s / |s|.
 *     x6d_out[p][j] = the first two columns of R(f), for j = 0 of R(conj(d_pair(p)) (x) f), in the 6-D layout of jrr_pose_smooth -- but
 *       when the only taken candidate is p itself, the row's six values bit for bit.
 *     dropped_out[p] = the number of joints at which p is a candidate and not taken.
 *     delta_orient_deg[p] = 2 atan2(|e_xyz|, |e_w|) 180 / pi of e = conj(q_p) (x) f at joint 0 (q'_p there);  delta_body_deg[p] = (the sum
 *       of those angles over the joints 1 .. 23, in joint order) / 23.
 *   betas_out[p] = (the sum over ALL members, ascending and starting from the first term) / (float)(number of members);
 *   members_out[p] = that number.  The camera translation is no output: it belongs to the view.
 *   A position's result depends on its group alone: not on m, the range or the launch's tiling.
 *   x6d_out_dev (m,24,6) 16-byte aligned, betas_out_dev (m,10), delta_*_deg_dev (m) float32, members_out_dev, dropped_out_dev (m) int32;
 *   rows outside the range are not touched.  Touches no engine.  No reference counterpart.                                      */
int jrr_view_relrot_accumulate(const float* table_dev, int64_t n_rows, const int32_t* order_dev, const int32_t* group_dev,
                               const int32_t* pair_dev, const int32_t* ref_pair_dev, int n_pairs, int m, int begin, int count,
                               int64_t* acc_dev, int32_t* status_dev, void* stream);
int jrr_view_fuse(const float* table_dev, int64_t n_rows, const int32_t* order_dev, const int32_t* group_dev, const int32_t* pair_dev,
                  const float* rel_dev, int n_pairs, int m, float cos_half_max, int begin, int count, float* x6d_out_dev,
                  float* betas_out_dev, float* delta_body_deg_dev, float* delta_orient_deg_dev, int32_t* members_out_dev,
                  int32_t* dropped_out_dev, int32_t* status_dev, void* stream);

/* find_joints, scripts/utils.py:85-103 (SMPL forward + J_regressor contraction).
 * Exactly one of x6d_dev (B,24,6) / R_dev (B,24,3,3) is non-NULL.  joints_dev (B,17,3).
 * verts_dev (B,6890,3) may be NULL (return_verts=False); non-NULL needs JRR_FLAG_KEEP_VERTS (or _SILHOUETTE):
 * the kernel stores the vertices coordinate-major and a transposing pass produces the reference's layout.  */
int jrr_find_joints_forward(jrr_engine_t* e, const float* x6d_dev, const float* R_dev,
                            const float* betas_dev, float* joints_dev, float* verts_dev, void* stream);
/* Adjoint of the call above for the SAME inputs (must follow it): djoints (B,17,3) ->
 * dx6d (B,24,6) or dR (B,24,3,3), dbetas (B,10), dJ (17,6890) w.r.t. the RAW J_regressor
 * (through the normalisation + ReLU + mask).  Any output pointer may be NULL.                 */
int jrr_find_joints_backward(jrr_engine_t* e, const float* x6d_dev, const float* R_dev,
                             const float* betas_dev, const float* djoints_dev, float* dx6d_dev,
                             float* dR_dev, float* dbetas_dev, float* dJ_dev, void* stream);

/* find_joints (scripts/utils.py:85-103) of the poses of the J step that PRECEDED -- jrr_j_regressor_grad[_support] followed by
 * jrr_j_step_apply[_support] on the same x6d / betas buffers, nothing else in between -- with the stepped regressor, re-regressed from
 * that step's stored vertices instead of a second SMPL forward: the joints the driver evaluates after the step
 * (scripts/optimize.py:317-321).  joints_dev (B,17,3).  A mismatch the engine can detect returns JRR_ERR_STATE.          */
int jrr_find_joints_after_j_step(jrr_engine_t* e, const float* x6d_dev, const float* betas_dev, float* joints_dev, void* stream);

/* The `joints` field of the SMPL operator's output (scripts/smpl.py:69-84: smplx's 24 posed joints J_transformed = G_j[:3, 3] of the
 * kinematic chain head the list the wrapper re-maps).  Must follow a forward on this engine (jrr_find_joints_forward,
 * jrr_refine_run, ...) with the SAME betas: reads the stored skinning transforms.  joints24_dev (B,24,3).
 * (dead on the hot path: every caller of the reference reads `.vertices` only).        */
int jrr_smpl_posed_joints(jrr_engine_t* e, const float* betas_dev, float* joints24_dev, void* stream);
/* Its adjoint (smplx's `joints` are differentiable, scripts/smpl.py:69-84): djoints24_dev (B,24,3) -> the gradients w.r.t. the forward's
 * inputs through the kinematic chain and the rest joints J(beta).  Exactly one of x6d_dev (B,24,6) / R_dev (B,24,3,3) names the rotation
 * input of that forward; outputs dx6d_dev (B,24,6) or dR_dev (B,24,3,3), and dbetas_dev (B,10), nullable.  Must follow the forward
 * like jrr_smpl_posed_joints.                                                                                          */
int jrr_smpl_posed_joints_backward(jrr_engine_t* e, const float* x6d_dev, const float* R_dev, const float* betas_dev,
                                   const float* djoints24_dev, float* dx6d_dev, float* dR_dev, float* dbetas_dev, void* stream);

/* SMPL operator on its own: smpl(global_orient, body_pose, betas, pose2rot=False).vertices
 * (call sites scripts/utils.py:94-95, scripts/optimize.py:78-79, scripts/renderer.py:32-33).
 * Forward = jrr_find_joints_forward with verts_dev != NULL.  This is the adjoint w.r.t. the
 * vertices for the SAME inputs (must follow that forward): dverts (B,6890,3) -> dx6d / dR, dbetas.
 * Needs JRR_FLAG_KEEP_VERTS (the padded vertex buffer doubles as the transposed adjoint).        */
int jrr_smpl_vertices_backward(jrr_engine_t* e, const float* x6d_dev, const float* R_dev,
                               const float* betas_dev, const float* dverts_dev, float* dx6d_dev,
                               float* dR_dev, float* dbetas_dev, void* stream);

/* move_pelvis + MSELoss, scripts/utils.py:106-114 + scripts/optimize.py:238-239:
 * sqerr_dev[b] = sum_{i,c} (joints[b,i,c]-joints[b,0,c] - gt_mm[b,i,c]/1000)^2 ;
 * djoints = d(weight * mean)/d joints with mean over batch_norm*51.                            */
int jrr_joint_loss(const float* joints_dev, const float* gt_centred_mm_dev, float weight,
                   int batch, int batch_norm, float* sqerr_dev, float* djoints_dev, void* stream);

/* Discriminator.forward, scripts/discriminator.py:32-54: x (B,24,6) -> out (B,25) sigmoid.    */
int jrr_pose_disc_forward(jrr_engine_t* e, const float* x6d_dev, float* out_dev, void* stream);
/* d[ weight * mean((D(x)-target)^2) ] / dx for the forward just run (optimize.py:246-247).    */
int jrr_pose_disc_backward_input(jrr_engine_t* e, const float* x6d_dev, float weight, float target,
                                 float* dx6d_dev, void* stream);
/* vector-Jacobian product of Discriminator.forward w.r.t. its input for an arbitrary upstream
 * gradient gout (B,25) (autograd backward of the module); must follow jrr_pose_disc_forward.   */
int jrr_pose_disc_vjp_input(jrr_engine_t* e, const float* x6d_dev, const float* gout_dev,
                            float* dx6d_dev, void* stream);
/* weight gradients of  mean((D(x)-target)^2)  (mean over batch_norm*25) accumulated (+=) into a
 * flat vector laid out like the parameter vector (one term of scripts/optimize.py:276-284);
 * sqerr_dev (B, nullable) receives sum_k (D(x)[b,k]-target)^2.                                   */
int jrr_pose_disc_backward_params(jrr_engine_t* e, const float* x6d_dev, float target,
                                  float* dparams_dev, float* sqerr_dev, void* stream);
/* vector-Jacobian product of Discriminator.forward w.r.t. the WEIGHTS for an arbitrary upstream gradient gout (B,25),
 * accumulated (+=) into a flat vector laid out like the parameter vector: what `loss.backward()` leaves in the
 * module's .grad for any loss of the discriminator output (scripts/optimize.py:276-284 through the nn.Module).  */
int jrr_pose_disc_vjp_params(jrr_engine_t* e, const float* x6d_dev, const float* gout_dev, float* dparams_dev,
                             void* stream);
/* the same for Shape_Discriminator: gout (B), 171 parameters (float atomics) */
int jrr_shape_disc_vjp_params(jrr_engine_t* e, const float* betas_dev, const float* gout_dev, float* dparams_dev,
                              void* stream);
/* the same for Shape_Discriminator (scripts/optimize.py:286-293): betas (B,10), 171 parameters */
int jrr_shape_disc_backward_params(jrr_engine_t* e, const float* betas_dev, float target,
                                   float* dparams_dev, float* sqerr_dev, void* stream);

/* Shape_Discriminator.forward, scripts/discriminator.py:70-74: betas (B,10) -> out (B) sigmoid scores; and the
 * vector-Jacobian product w.r.t. the input for an upstream gradient gout (B) (autograd backward of the module).
 * Stateless apart from the parameters (jrr_engine_set_shape_disc): the vjp recomputes the 171-parameter forward. */
int jrr_shape_disc_forward(jrr_engine_t* e, const float* betas_dev, float* out_dev, void* stream);
int jrr_shape_disc_vjp_input(jrr_engine_t* e, const float* betas_dev, const float* gout_dev, float* dbetas_dev,
                             void* stream);

/* torch.optim.Adam single-tensor update (defaults used at scripts/optimize.py:116-126,201):
 * step_dev holds the 1-based step count of THIS update.                                        */
int jrr_adam_step(float* p_dev, const float* g_dev, float* m_dev, float* v_dev, size_t n,
                  const int32_t* step_dev, float lr, float beta1, float beta2, float eps, void* stream);

/* evaluate, scripts/utils.py:117-145 + scripts/eval_utils.py:7-58 (row f3): per-pose mean joint error and
 * Procrustes-aligned mean joint error in METRES (pred in m, target in mm, both pelvis-centred inside);
 * MPJPE / PA-MPJPE in mm = 1000 * mean over poses.
 * The alignment is the reference's torch.svd + det-sign fix, degenerate shapes included.  The 3x3 SVD of K = X1 X2^T is a
 * one-sided (Hestenes) Jacobi iteration on K itself (K^T K is never formed), the rotation v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T:
 *   rank 3 and rank 2 (a flat pred and/or target, mirrored or not): the unique proper rotation of the reference;
 *   rank 1 (a pred or a target on a line, sigma_2 <= 1e-6 sigma_1): the rotation about the line is free, the aligned distances are not;
 *   rank 0: a constant target gives aligned distances of exactly 0, a constant pred NaN (the reference's 0/0) in its own aligned
 *           values only, its plain distances stay finite.
 * One pose per thread, no cross-lane arithmetic: a pose's result does not depend on the other poses of the batch.        */
int jrr_evaluate(const float* pred_j3d_dev, const float* target_j3d_mm_dev, float* err_dev, float* err_pa_dev,
                 int batch, void* stream);

/* evaluate WITHOUT its mean over the joints (scripts/utils.py:127-138 + scripts/eval_utils.py:7-58): err_j_dev / err_pa_j_dev
 * (batch,17), the per-joint distance and Procrustes-aligned distance in METRES of which jrr_evaluate returns the means (same
 * arithmetic: one shared body).  pred in m, target in mm, both pelvis-centred inside.  Both outputs 16-byte aligned.          */
int jrr_evaluate_joints(const float* pred_j3d_dev, const float* target_j3d_mm_dev, float* err_j_dev, float* err_pa_j_dev,
                        int batch, void* stream);

/* Joints of meshes that need not come from this library: what scripts/test.py:206-212,255-283 (test_pose_refiner_model_VIBE_MEVA)
 * and :362-373 (METRO) do with another model's vertices, with the arithmetic of find_joints (scripts/utils.py:87-98).
 * jrr_regress_joints_prepare, once per set of regressors: J_dev (n_reg,17,6890) raw, 1 <= n_reg <= JRR_REGRESS_MAX_REG; mask_dev
 * (17,6890) or NULL.  J*mask, ReLU, division of each row by its sum, and each row's list of positive columns in ascending order,
 * into workspace_dev (caller-owned, 16-byte aligned, jrr_regress_joints_workspace_bytes(n_reg) bytes).  One table serves any
 * number of batches.
 * jrr_regress_joints: verts_dev (batch,6890,3) pose-major fp32, 8-byte aligned; joints_dev (n_reg,batch,17,3).  The vertices are
 * read once for all n_reg regressors.  Every output is summed over its row's list in ONE fixed order (double accumulation, one
 * rounding): it does not depend on batch, on n_reg or on the launch.  A row whose sum is zero gives NaN for that joint of that
 * regressor (the reference's 0/0) and disturbs nothing else.  n_reg must be the prepared one.                                  */
size_t jrr_regress_joints_workspace_bytes(int n_reg);
int jrr_regress_joints_prepare(const float* J_dev, int n_reg, const float* mask_dev, void* workspace_dev, size_t workspace_bytes,
                               void* stream);
int jrr_regress_joints(const float* verts_dev, int batch, const void* workspace_dev, int n_reg, float* joints_dev, void* stream);

/* The evaluation report's accumulator (no reference counterpart: scripts/test.py:125-138 prints four means; the per-joint,
 * per-action and PCK / AUC numbers are read from this table).  ADDS the poses of err_j_dev / err_pa_j_dev (batch,17) to rows
 * group_dev[b] of acc_dev: int64 [n_groups][JRR_EVAL_ACC_ROW] + JRR_EVAL_ACC_TRAILER words, layout above; the caller zeroes it
 * once per report.  1 <= n_groups <= JRR_EVAL_ACC_MAX_GROUPS.  A pose with a value that fails e < 1.0e3f counts in word 1 of its
 * row only (the cap keeps int64 from overflowing below ~5e8 poses; it is no tolerance); group < 0 counts in trailer word 0 only,
 * group >= n_groups in trailer word 1 only.  Integer atomics only: the table does not depend on the order, on the split into
 * calls or on the sharding over ranks (sum the ranks' tables).                                                              */
int jrr_eval_accumulate(const float* err_j_dev, const float* err_pa_j_dev, const int32_t* group_dev, int batch, int n_groups,
                        int64_t* acc_dev, void* stream);

/* The evaluation report under a published protocol (`--eval_protocol`; no reference counterpart in running code: H36M_TO_J14 of
 * scripts/constants.py and the commented METRO block name the 14 joints): which joints are scored, where both skeletons are centred,
 * in which unit the target comes.  One launch.  M = the joints whose bit is set in joint_mask, ascending, n = |M|.  Per pose, fp32:
 *   target   Q_i = target_i / 1000.f under JRR_EVAL_TARGET_MM (exactly as jrr_evaluate_joints), target_i itself under JRR_EVAL_TARGET_M
 *   root     JRR_EVAL_ROOT_JOINT0: rP = P_0, rQ = Q_0; JRR_EVAL_ROOT_HIPS: rP_c = (P_1c + P_4c) * 0.5f, rQ likewise.  The root joints are
 *            used whether or not they are in M.
 *   plain    for i in M: P_i -= rP, Q_i -= rQ, err_j[i] = |P_i - Q_i|
 *   aligned  the Procrustes fit of jrr_evaluate_joints over M ALONE: means divided by (float)n, K and var1 summed over M in ascending
 *            order, the same one-sided Jacobi (six sweeps), static sort and rank-2 / rank-1 / rank-0 rules;
 *            err_pa_j[i] = |s R P_i + t - Q_i| for i in M.  A single joint (var1 = 0) gives NaN there, as the reference does.
 *   others   a joint outside M gets +0.0f in both outputs.  A joint that is neither in M nor a root joint is not read: a NaN there
 *            changes no output bit.
 * err_j_dev / err_pa_j_dev (batch,17) metres, each nullable, 16-byte aligned.  With zeros in the excluded columns a sum over the 17
 * columns is a sum over the protocol's joints: jrr_paired_units takes these arrays UNCHANGED (its four sums are then sums over M, and a
 * zero passes its e < 1.0e3f test).  They are NOT input for jrr_eval_accumulate: its histograms would count the zeros of the excluded
 * joints in bin 0 and its COUNT-based divisor is 17.  Use acc_dev here instead:
 * acc_dev (nullable) is the table of jrr_eval_accumulate (JRR_EVAL_ACC_*, n_groups rows + the 2-word trailer), added to in the same
 * launch with that function's expressions: group_dev (batch) int32 or NULL (every pose in group 0); group < 0 counts in trailer word 0
 * only, group >= n_groups in trailer word 1 only; a pose with a value OF A JOINT IN M failing e < 1.0e3f adds BAD += 1 only; otherwise
 * COUNT += 1 and, for i in M only, SUM[i], SUM_PA[i] and one bin each of HIST and HIST_PA.  The words of excluded joints stay 0, so the
 * means are sum / (n COUNT) and PCK = (bins below t) / (n COUNT).  Integer atomics only: the table is a function of the multiset of
 * (pose, group) pairs.  At JRR_EVAL_MASK_ALL, JRR_EVAL_ROOT_JOINT0, JRR_EVAL_TARGET_MM the table equals what jrr_eval_accumulate makes of
 * the two arrays written here.  One pose per thread, no value crosses lanes: a pose's result does not depend on batch or on its place.
 * JRR_ERR_ARG with a message, before any launch: a NULL pred or target; all three outputs NULL; joint_mask == 0 or a bit at or above
 * 17; an unknown root or unit; batch < 0; n_groups outside 1 .. JRR_EVAL_ACC_MAX_GROUPS with acc_dev given; a misaligned array.
 * batch == 0 returns JRR_OK without a launch.                                                                                       */
enum { JRR_EVAL_ROOT_JOINT0 = 0, JRR_EVAL_ROOT_HIPS = 1 };      /* hips: midpoint of joints 1 and 4 */
enum { JRR_EVAL_TARGET_MM = 0, JRR_EVAL_TARGET_M = 1 };
enum { JRR_EVAL_MASK_ALL = 0x1FFFF, JRR_EVAL_MASK_LSP14 = 0x1FD7E };      /* LSP14: the 17 minus Pelvis (0), Torso (7) and Nose (9) */
int jrr_evaluate_protocol(const float* pred_dev /* (batch,17,3) m */, const float* target_dev /* (batch,17,3) */, int target_unit,
                          uint32_t joint_mask, int root, const int32_t* group_dev /* (batch) or NULL: group 0 */, int batch, int n_groups,
                          float* err_j_dev, float* err_pa_j_dev /* (batch,17) m, each nullable */, int64_t* acc_dev /* nullable */,
                          void* stream);

/* The acceleration error along each video sequence (`--eval_accel`; the HMMR / VIBE convention, no reference counterpart in code:
 * this text is the specification).  pred_dev (n_rows,17,3) fp32 metres and gt_mm_dev (n_rows,17,3) fp32 millimetres are tables whose
 * row is the dataset index; both are only read.  order_dev (m) int32 lists table rows in time order and run_dev (m) int32 gives each
 * position's run of consecutive frames of one camera (the host forms both from the frame paths, as for jrr_pose_smooth); group_dev
 * (m) int32 or NULL (every position in group 0) is each position's group.  A position p has a TRIPLE when 0 <= p - 1, p + 1 < m,
 * run[p - 1] == run[p] == run[p + 1] and none of the three is absent (below): not the first or last of its run, no run shorter than 3.
 * The neighbours are looked up in the whole list [0, m), whatever the range.  Per frame of the triple, as jrr_evaluate centres its
 * inputs: x = P - P[0], y = G / 1000 - (G / 1000)[0].  Per joint j and component:
 *   a_pred = (x[p-1] - 2 x[p]) + x[p+1], a_gt the same expression on y;  e_j = |a_pred - a_gt|, s_j = |a_pred|, g_j = |a_gt|,
 *   |v| = sqrtf((v0 v0 + v1 v1) + v2 v2): metres per sampled frame^2.
 * Every operation is rounded once in fp32, in the order written; no product is fused into a sum.
 *   begin, count   the positions [begin, begin + count) the call computes.  The per-position outputs err_j_dev, acc_pred_j_dev,
 *                  acc_gt_j_dev (m,17) fp32 -- e_j, s_j, g_j; each may be NULL -- are indexed by position and the other rows are not
 *                  touched.  A position without a triple gets 17 NaN in each.  A result depends on its triple alone: not on m, the
 *                  range or the launch's tiling (JRR_ACCEL_TILE positions per workgroup).
 *   acc_dev        NULL, or int64 [n_groups][JRR_ACCEL_ACC_ROW] + JRR_ACCEL_ACC_TRAILER words, layout above, to which the call ADDS
 *                  its positions; the caller zeroes it once per report.  1 <= n_groups <= JRR_EVAL_ACC_MAX_GROUPS.  A position adds
 *                  to exactly one word class: group < 0 to trailer word 0 only; group >= n_groups to trailer word 1 only (the caller's
 *                  error); otherwise, in row group[p]: without a triple NO_TRIPLE += 1 only; with one of the 51 values e_j, s_j, g_j
 *                  failing v < 1.0e3f (NaN, inf; a guard against overflow, no tolerance) BAD += 1 only -- its per-position outputs
 *                  still hold what was computed --; else COUNT += 1 and per joint SUM_ERR += llrintf(e_j * 2^24), SUM_PRED +=
 *                  llrintf(s_j * 2^24), SUM_GT += llrintf(g_j * 2^24), HIST[min((int)floorf(e_j * 1000.f), 150)] += 1.
 *                  Integer atomics only: the table is a function of the multiset of positions -- not of the order, the split into
 *                  calls or the sharding over ranks (sum the ranks' tables).
 *   status_dev     one int32 the CALLER zeroes and reads when it next synchronises: bit 0 (JRR_ACCEL_STATUS_INDEX) an entry of order
 *                  outside [0, n_rows).  Such a position is ABSENT: it forms no triple (NaN outputs, NO_TRIPLE) and is nobody's
 *                  neighbour; every other position is unaffected.
 * count == 0 returns JRR_OK without a launch.  JRR_ERR_ARG with a message: a NULL pred / gt_mm / order / run / status, a negative
 * size, a range outside [0, m), all four outputs NULL, n_groups out of range with acc_dev given, a misaligned array (4 bytes, acc_dev 8).
 * Touches no engine.                                                                                                         */
int jrr_accel_error(const float* pred_dev, const float* gt_mm_dev, int64_t n_rows, const int32_t* order_dev, const int32_t* run_dev,
                    const int32_t* group_dev, int m, int begin, int count, int n_groups, float* err_j_dev, float* acc_pred_j_dev,
                    float* acc_gt_j_dev, int64_t* acc_dev, int32_t* status_dev, void* stream);

/* The per-vertex error of meshes (`--eval_pve`): PVE / MPVPE and its Procrustes-aligned form PA-PVE, the fourth column mesh-recovery
 * papers print.  pred_dev and gt_dev are (batch,n_verts,3) fp32 METRES, both; root_pred_dev / root_gt_dev (batch,3) or NULL (zero) are
 * subtracted first; 1 <= n_verts <= JRR_PVE_MAX_VERTS.  Per pose b, every fp32 operation rounded once in the order written, no product
 * fused into a sum:
 *   x_i = P_i - root_pred, y_i = Q_i - root_gt;  d_i = sqrtf((dx dx + dy dy) + dz dz) of x_i - y_i.
 *   Procrustes (scripts/eval_utils.py:7-58 of the reference on all vertices): from the fp32 x_i, y_i IN DOUBLE the means mu1, mu2, then
 *   K = sum (x_i - mu1)(y_i - mu2)^T and var1 = sum ((a0 a0 + a1 a1) + a2 a2), a = x_i - mu1, about the double means.  The order of
 *   the double sums is a function of n_verts alone (vertex i belongs to thread i mod 256, which adds its vertices in ascending order;
 *   the 64 sums of a wave are combined by an xor butterfly over lane distances 32, 16, ..., 1; the 4 wave sums are added in wave
 *   order).  mu1, mu2, K, var1 are each rounded to fp32; the rotation, scale = trace(R K) / var1 and t = mu2 - scale R mu1 are those
 *   of jrr_evaluate, statement by statement (one-sided Jacobi on K, six sweeps, the sort, the rank-1 and rank-0 rules);
 *   e_i = |scale R x_i + t - y_i|, h_r = scale * ((R_r0 x_0 + R_r1 x_1) + R_r2 x_2) + t_r.  A constant target gives e_i == 0 exactly; a
 *   constant pred (also n_verts == 1) gives NaN in e only.
 *   q_i = llrintf(d_i * 2^24), S = sum q_i (int64, exact), pve = (float)((double)S / ((double)n_verts * 16777216.0)); pve = NaN when
 *   a d_i fails d_i < 1.0e3f.  The same on e_i gives pa_pve.
 *   pve_dev, pa_pve_dev   (batch) fp32 metres, each may be NULL
 *   err_v_dev, err_pa_v_dev   (batch,n_verts) fp32: d_i, e_i as computed, each may be NULL
 *   acc_dev     NULL, or int64 [n_groups][JRR_PVE_ACC_ROW] + JRR_PVE_ACC_TRAILER words, layout above, to which the call ADDS its poses
 *               by group_dev (batch) int32 (NULL: every pose in group 0); the caller zeroes it once per report.  group < 0 counts in
 *               trailer word 0 only, group >= n_groups in trailer word 1 only.  Otherwise: a pose with either mean NaN adds BAD += 1 and
 *               nothing else; else COUNT += 1, SUM += llrintf(pve * 2^24), SUM_PA likewise, HIST[min((int)floorf(pve * 1000.f), 150)]
 *               += 1, HIST_PA likewise, and per part p with part_dev (n_verts) int32 labels given, 1 <= n_parts <= JRR_PVE_MAX_PARTS:
 *               PART[p] += llrintf(m_p * 2^24), m_p = (float)((double)(sum of q_i over part_dev[i] == p) / ((double)n_p * 16777216.0)),
 *               n_p the part's vertex count; PART_PA likewise.  Empty parts and labels outside [0, n_parts) add nothing.
 *   acc_v_dev   NULL, or int64 [2][n_verts], to which the call ADDS q_i (plain, then aligned) of every counted pose: one whose means
 *               are both no NaN and whose group lies in [0, n_groups) (group_dev NULL: every such pose).
 * Integer atomics only: the tables are a function of the multiset of (pose, group) pairs -- not of the order, the split into calls or
 * the sharding over ranks (sum the ranks' tables).  A pose's outputs do not depend on batch or on its place in the batch.
 * batch == 0 returns JRR_OK without a launch.  JRR_ERR_ARG with a message, nothing touched: a NULL pred / gt, all six outputs NULL,
 * batch < 0, n_verts out of range, part_dev without 1 <= n_parts <= 32, n_groups outside 1 .. JRR_EVAL_ACC_MAX_GROUPS with acc_dev (or
 * with acc_v_dev and group_dev), a misaligned array (4 bytes; acc_dev, acc_v_dev 8).  Touches no engine and no body model.       */
int jrr_vertex_error(const float* pred_dev, const float* gt_dev, const float* root_pred_dev, const float* root_gt_dev,
                     const int32_t* group_dev, const int32_t* part_dev, int n_parts, int batch, int n_verts, int n_groups,
                     float* pve_dev, float* pa_pve_dev, float* err_v_dev, float* err_pa_v_dev, int64_t* acc_dev, int64_t* acc_v_dev,
                     void* stream);

/* The paired bootstrap of the evaluation report (`--eval_ci`; no reference counterpart: scripts/test.py:125-138 prints four means and
 * no word on how sure their difference is).  Tables: JRR_BOOT_* above.
 *
 * jrr_paired_units: the four (batch,17) fp32 arrays jrr_evaluate_joints wrote -- plain and aligned errors of the initial regressor
 * (before_dev, before_pa_dev) and of the retrained one (after_dev, after_pa_dev) on the SAME poses -- with group_dev and unit_dev
 * (batch) int32.  Per pose, four int64 sums S_c = sum_j rn(e_j * 2^24): the expression of jrr_eval_accumulate, from one shared header,
 * so per group the column sums of the units equal the sums over j of that table's SUM words.  A pose adds to exactly one word class:
 * group < 0 to trailer word IGNORED only; group >= n_groups to BAD_GROUP only; else a unit outside [0, n_units) to BAD_UNIT only;
 * else, with one of its 68 values failing e < 1.0e3f (NaN, inf; a guard against overflow, no tolerance), to its group's BAD only -- the
 * analysis is paired: a pose that is bad for one regressor is out for both --; else S_before, S_before_pa, S_after, S_after_pa, 1 to
 * units_dev[unit] and, in wins_dev[group], COUNT += 1 and one of BETTER / WORSE / TIE by the integer comparison of S_after with
 * S_before, and one of the three _PA words likewise.  Integer atomics only: the tables are a function of the multiset of poses -- not
 * of the order, the split into calls or the sharding over ranks (sum the ranks' tables).  The caller zeroes both tables once per
 * report; nothing is read back.  1 <= n_groups <= JRR_EVAL_ACC_MAX_GROUPS, n_units >= 1; batch == 0 returns JRR_OK without a launch.
 *
 * jrr_bootstrap_sums: units_dev int64 [n_units][5]; segments_host int32 [n_seg][2] = (begin, count) runs of unit rows, in HOST
 * memory: the call checks them and then uploads these very words to segments_dev (n_seg * 2 int32 of device memory the caller owns), so
 * the launch reads what was checked.  out_dev int64 [n_seg][rep_count][5]: row (s, r - rep_begin) is the sum of count_s unit rows,
 * draw i of which is row begin_s + ((w * count_s) >> 32) with w the word i & 3 of Philox4x32-10 at counter (i >> 2, r, s, 0) under
 * key (seed & 0xffffffff, seed >> 32), for replicates r = rep_begin .. rep_begin + rep_count - 1 (multipliers 0xD2511F53 and
 * 0xCD9E8D57, Weyl constants 0x9E3779B9 and 0xBB67AE85).  A segment with count 0 gives a zero row.  Every output word is stored exactly
 * once: no atomics, nothing to zero.  A row depends on (seed, r, s, begin_s, count_s) and the unit rows alone: not on the launch, on
 * rep_begin, on rep_count or on the other segments, so the replicates may be split over calls and over ranks.
 * JRR_ERR_SEGMENT, with a message and without a launch: a negative count, a segment that leaves [0, n_units).  JRR_ERR_ARG: a NULL
 * pointer, n_seg outside 1 .. JRR_BOOT_MAX_SEGMENTS, a negative replicate range or one that reaches 2^31, a misaligned table.
 * rep_count == 0 returns JRR_OK without a launch.  The caller keeps the sums below 2^63: the overflow rule at JRR_BOOT_*.          */
int jrr_paired_units(const float* before_dev, const float* before_pa_dev, const float* after_dev, const float* after_pa_dev,
                     const int32_t* group_dev, const int32_t* unit_dev, int batch, int n_groups, int n_units, int64_t* units_dev,
                     int64_t* wins_dev, void* stream);
int jrr_bootstrap_sums(const int64_t* units_dev, int n_units, const int32_t* segments_host, int32_t* segments_dev, int n_seg, uint64_t seed,
                       int rep_begin, int rep_count, int64_t* out_dev, void* stream);

/* ---- regressor report (`--regressor_report`): how far the retrained regressor moved each joint, and discs on a picture ------
 * No reference counterpart in code: the reference's teaser.png shows the joints of the accepted regressor, of the retrained one and
 * the ground truth on the fitted mesh; scripts/test.py:107-123 regresses both sets and keeps only their errors.
 *
 * jrr_regressor_shift_accumulate ADDS the poses of joints_a_dev / joints_b_dev (batch,17,3) fp32 metres -- regressor A (initial) and B
 * (retrained) on the same meshes, as the regressors produce them, not pelvis-centred -- to rows group_dev[b] of acc_dev: int64
 * [n_groups][JRR_SHIFT_ACC_ROW] + JRR_SHIFT_ACC_TRAILER words, layout above; the caller zeroes it once per report.  group_dev NULL:
 * every pose in group 0.  group < 0 counts in trailer word 0 only, group >= n_groups in trailer word 1 only, as in
 * jrr_eval_accumulate; 1 <= n_groups <= JRR_EVAL_ACC_MAX_GROUPS.
 * Per pose, every operation rounded once in fp32 in the order written, no product fused into a sum (a . b = (a0 b0 + a1 b1) + a2 b2,
 * |a| = sqrtf(a . a), a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)), a[i] the joints of A:
 *   x = a[4] - a[1] (L_Hip - R_Hip), u = a[8] - a[0] (Neck - Pelvis); xh = x / |x|; z = xh x u; zh = z / |z|; yh = zh x xh
 *     (an upright SMPL body gives the identity: x to the body's left, y up, z forward)
 *   per joint j: d = b[j] - a[j]; c = (d . xh, d . yh, d . zh); q = llrintf(c * 2^24); len = |d|; r = d - d[0], rel = |r|
 * The pose counts in JRR_SHIFT_ACC_BAD only, and adds nothing else, when one of its 102 inputs is non-finite, or !(|x| >= 1e-4f), or
 * !(|z| >= 1e-4f * |u|), or one of the 51 components fails |c| < 4.0f.  Otherwise COUNT += 1 and per joint SUM += q, MOM += (q_i q_j) >> 16,
 * ABS += llrintf(len * 2^24), ABS_REL += llrintf(rel * 2^24), HIST[min(63, (int)floorf(len * 500.0f))] += 1.
 * Integer atomics only: the table is a function of the multiset of (pose, group) pairs -- not of the order, the split into calls or
 * the sharding over ranks (sum the ranks' tables).                                                                          */
int jrr_regressor_shift_accumulate(const float* joints_a_dev, const float* joints_b_dev, const int32_t* group_dev, int batch,
                                   int n_groups, int64_t* acc_dev, void* stream);
/* jrr_draw_discs paints filled discs INTO an existing picture rgb_dev (batch,h,w,3) uint8, interleaved, any h, w >= 1 (h * w <= 2^28).
 *   points_dev   (n_sets,batch,n_pts,2) fp32 (x, y) in the picture's pixel frame
 *   radius_dev   (n_sets,batch,n_pts) fp32 or NULL: then every disc has the scalar `radius`
 *   colours_host (n_sets,3) uint8
 *   1 <= n_sets <= JRR_DISCS_MAX_SETS, 1 <= n_pts <= JRR_DISCS_MAX_POINTS; anything else returns JRR_ERR_ARG and touches nothing.
 * The inside rule is jrr_fit_overlay's: pixel (x, y) has its centre at the integer coordinate and is inside the disc (px, py, r) iff
 * dx * dx + dy * dy <= r * r with dx = (float)x - px, dy = (float)y - py, every term rounded once in fp32.  A later set paints over an
 * earlier one, within a set a later point over an earlier one.  A point with a non-finite coordinate or radius, or r < 0, draws
 * nothing (r = 0 at an exact pixel centre draws that pixel); discs are clipped to the picture; a pixel outside every disc keeps its
 * bytes (it is not written).  One thread owns a pixel and walks the points in order: no atomics, the result is a function of the
 * inputs alone.                                                                                                              */
int jrr_draw_discs(uint8_t* rgb_dev, int batch, int h, int w, const float* points_dev, const float* radius_dev, float radius,
                   const uint8_t* colours_host, int n_sets, int n_pts, void* stream);

/* ---- depth below the skin (`--regressor_report_depth`): is a regressed joint inside the body, and how deep -------------------
 * No reference counterpart: a row of the regressor lies on the simplex, so its joint lies in the convex hull of its support vertices,
 * which is not the body; scripts/test.py:107-123 regresses the joints and never asks where they are.
 *
 * jrr_point_mesh_depth: for each pose b of verts_dev (batch,n_verts,3) fp32 metres and each point p of points_dev (batch,n_points,3),
 * against the triangles faces_dev (n_faces,3) int32 that all poses share -- with a face's corners a, b, c and A = a - p, B = b - p,
 * C = c - p, everything in fp32 unless said otherwise (products may be fused into sums):
 *   dist_dev (batch,n_points)  the minimum over the faces of the Euclidean distance from p to the closest point of the closed
 *       triangle, >= 0.  The closest point lies in one of seven regions -- corner a, b or c, edge ab, ac or bc, the interior -- found
 *       from d1 = ab . ap, d2 = ac . ap, d3 = ab . bp, d4 = ac . bp, d5 = ab . cp, d6 = ac . cp (ab = b - a, ac = c - a, ap = -A,
 *       bp = -B, cp = -C), vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4; the first region that holds, in this order:
 *         a: d1 <= 0 and d2 <= 0;  b: d3 >= 0 and d4 <= d3;  ab: vc <= 0, d1 >= 0, d3 <= 0, at a + ab d1 / (d1 - d3);
 *         c: d6 >= 0 and d5 <= d6;  ac: vb <= 0, d2 >= 0, d6 <= 0, at a + ac d2 / (d2 - d6);
 *         bc: va <= 0, d4 - d3 >= 0, d5 - d6 >= 0, at b + (c - b) (d4 - d3) / ((d4 - d3) + (d5 - d6));
 *         interior: a + ab vb / (va + vb + vc) + ac vc / (va + vb + vc).
 *       A corner region takes A, B or C itself as the offset, the others A + v ab + u ac.  The value compared between faces is the
 *       squared length of the offset; dist is the square root of the smallest.
 *   face_dev (batch,n_points)  a face that attains it: among equal computed squared lengths the smallest index.  A face whose
 *       computed value is NaN (zero area: 0 / 0) never wins.  -1 when no face gave a value.
 *   wind_dev (batch,n_points)  the winding number of the surface around p, (sum over the faces of Omega) / 4 pi with
 *       Omega = 2 atan2f(A . (B x C), |A||B||C| + (A . B)|C| + (B . C)|A| + (C . A)|B|)   (van Oosterom and Strackee).
 *       Each Omega is formed in fp32; the Omega are summed in double and the quotient is rounded to float once.  The order of the
 *       sum is a function of n_faces alone: face f goes to partial sum f mod 16, each partial sum adds its faces in ascending order,
 *       and the sixteen are added as the balanced tree ((s0 + s1) + (s2 + s3)) + ... .  Nothing depends on batch, on the pose's
 *       position in the batch, on n_points or on the point's index: a pose gives the same bits alone and inside a batch, a point the
 *       same bits in any column.  A closed surface gives an integer, 0 outside; the callers' rule is inside <=> fabsf(wind) > 0.5f.
 *       The sign is the orientation of the faces (the synthetic body gives -1 inside): nothing may assume +1.
 *   Any of the three outputs may be NULL (not all three).
 * A face with an index outside [0, n_verts) is skipped for both quantities and sets bit 0 (JRR_DEPTH_STATUS_INDEX) of status_dev[0],
 * which the caller zeroes and reads at its next synchronise.  A pose with a non-finite value among its n_verts vertices gives NaN
 * dist, NaN wind and face -1 for all of its points; a point with a non-finite coordinate gives them for itself.  Neither disturbs
 * another pose or another point.
 * Limits: 1 <= n_points <= JRR_DEPTH_MAX_POINTS, 1 <= n_verts <= JRR_DEPTH_MAX_VERTS, 1 <= n_faces; verts_dev 8-byte aligned.
 * JRR_ERR_ARG with a message, and no launch: a NULL input or status, all three outputs NULL, a size out of range, a misaligned pointer.
 * batch == 0 returns JRR_OK without a launch.  No engine is touched.                                                          */
int jrr_point_mesh_depth(const float* verts_dev, int batch, int n_verts, const int32_t* faces_dev, int n_faces, const float* points_dev,
                         int n_points, float* dist_dev, float* wind_dev, int32_t* face_dev, int32_t* status_dev, void* stream);
/* jrr_depth_accumulate ADDS the poses of dist_dev / wind_dev (batch,n_points), as jrr_point_mesh_depth wrote them, to rows group_dev[b]
 * of acc_dev: int64 [n_groups][JRR_DEPTH_ACC_ROW] + JRR_DEPTH_ACC_TRAILER words, layout above; the caller zeroes it once per report.
 * group_dev NULL: every pose in group 0.  group < 0 counts in trailer word 0 only, group >= n_groups in trailer word 1 only, as in
 * jrr_eval_accumulate; 1 <= n_groups <= JRR_EVAL_ACC_MAX_GROUPS, 1 <= n_points <= JRR_DEPTH_MAX_POINTS.
 * A pose counts in JRR_DEPTH_ACC_BAD only, and adds nothing else, when one of its 2 n_points values is non-finite or one of its dist
 * fails d < 1.0e3f (the project's overflow cap, no tolerance).  Otherwise COUNT += 1 and per point column k < n_points, every
 * operation rounded once in fp32 in the order written: inside = fabsf(wind) > 0.5f; depth = inside ? dist : -dist;
 * OUTSIDE[k] += !inside; UNSURE[k] += fabsf(fabsf(wind) - rintf(fabsf(wind))) > 0.1f; SUM[k] += llrintf(depth * 2^24);
 * HIST[k][max(0, min(63, (int)floorf((depth + 0.064f) * 250.0f)))] += 1.  Columns k >= n_points are not touched.
 * Integer atomics only: the table is a function of the multiset of (pose, group) pairs -- not of the order, the split into calls or
 * the sharding over ranks (sum the ranks' tables).                                                                          */
int jrr_depth_accumulate(const float* dist_dev, const float* wind_dev, const int32_t* group_dev, int batch, int n_points, int n_groups,
                         int64_t* acc_dev, void* stream);

/* ---- self-penetration of a mesh (`--eval_penetration`): is it a possible body at all -----------------------------------------------
 * No reference counterpart.  A vertex pushed a little under the skin, x - offset * (outward normal), has an integer winding number of
 * the closed surface around it: 1 for sound skin, 2 or more where that piece of skin lies inside another piece of the body (an arm
 * through the chest), 0 where the body is thinner than the push.  No closest face, no part heuristics, no tree: the winding number at
 * every vertex, n_verts * n_faces solid angles per pose.
 *
 * jrr_mesh_winding: wind_dev (batch,n_points) = the `wind` of jrr_point_mesh_depth for the poses verts_dev (batch,n_verts,3), the
 * triangles faces_dev (n_faces,3) int32 they share and the points points_dev (batch,n_points,3), many points per pose: the same Omega
 * (van Oosterom and Strackee, each Omega formed in fp32, products may be fused into sums), summed in double, divided by 4 pi and
 * rounded to float once.  The order of the sum is a function of n_faces alone: face f goes to partial sum f mod 4, each partial sum
 * adds its faces in ascending order, and the four are added as (s0 + s1) + (s2 + s3).  (jrr_point_mesh_depth sums in another order:
 * the two calls agree within rounding, not in bits.)  Nothing depends on batch, on the pose's position in the batch, on n_points, on
 * the point's index or on how the launch tiles the points: a point gives the same bits alone and inside a batch, in any column.  The
 * sign is the orientation of the faces (the synthetic body gives -1 inside): nothing may assume +1.
 * A face with an index outside [0, n_verts) is skipped and sets bit 0 (JRR_DEPTH_STATUS_INDEX) of status_dev[0], which the caller
 * zeroes and reads at its next synchronise.  A pose with a non-finite value among its n_verts vertices gives NaN for all of its
 * points; a point with a non-finite coordinate gives NaN for itself.  Neither disturbs another pose or another point.
 * Limits: 1 <= n_points <= JRR_WINDING_MAX_POINTS (n_points need not be n_verts), 1 <= n_verts <= JRR_DEPTH_MAX_VERTS, 1 <= n_faces.
 * JRR_ERR_ARG with a message, and no launch: a NULL pointer, batch < 0, a size out of range, a pointer not 4-byte aligned.
 * batch == 0 returns JRR_OK without a launch.  No engine is touched.                                                          */
int jrr_mesh_winding(const float* verts_dev, int batch, int n_verts, const int32_t* faces_dev, int n_faces, const float* points_dev,
                     int n_points, float* wind_dev, int32_t* status_dev, void* stream);
/* jrr_penetration_accumulate: wind_dev (batch,n_verts) as jrr_mesh_winding wrote it for the pushed vertices.  Per value w, in fp32,
 * every operation rounded once: aw = fabsf(w), k = rintf(aw); PENETRATING: k >= 2.f; THIN: k == 0.f; UNSURE: fabsf(aw - k) > 0.1f (a
 * NaN is none of the three).  n_pen_dev, n_thin_dev, n_unsure_dev (batch) int32, each nullable: the counts of the pose's vertices,
 * written for EVERY pose, whatever its group.
 * The pose is then ADDED to row group_dev[b] of acc_dev: int64 [n_groups][JRR_PEN_ACC_ROW] + JRR_PEN_ACC_TRAILER words, layout above;
 * the caller zeroes it once per report.  group_dev NULL: every pose in group 0.  group < 0 counts in trailer word 0 only,
 * group >= n_groups in trailer word 1 only, as in jrr_depth_accumulate; 1 <= n_groups <= JRR_EVAL_ACC_MAX_GROUPS,
 * 1 <= n_verts <= JRR_WINDING_MAX_POINTS.  A pose with a non-finite wind value counts in JRR_PEN_ACC_BAD only.  Otherwise COUNT += 1,
 * POSES_PEN += n_pen >= 1, POSES_PEN8 += n_pen >= 8, SUM_PEN += n_pen, SUM_THIN += n_thin, SUM_UNSURE += n_unsure,
 * HIST[min(15, number of bits of n_pen)] += 1 (bin 0: n_pen == 0), and for every penetrating vertex v: PART[l] += 1 with l = part_dev[v]
 * (n_verts int32; a label outside [0, 32) counts as 31; part_dev NULL: 0) and per_vertex_dev[v] += 1 (n_verts int64, nullable, zeroed
 * by the caller once per report).
 * Integer atomics only: the tables are functions of the multiset of (pose, group) pairs -- not of the order, the split into calls or
 * the sharding over ranks (sum the ranks' tables).  JRR_ERR_ARG with a message, and no launch: wind_dev or acc_dev NULL, batch < 0, a
 * size out of range, a table not 8-byte or another pointer not 4-byte aligned.  batch == 0 returns JRR_OK without a launch.    */
int jrr_penetration_accumulate(const float* wind_dev, const int32_t* part_dev, const int32_t* group_dev, int batch, int n_verts,
                               int n_groups, int64_t* acc_dev, int64_t* per_vertex_dev, int32_t* n_pen_dev, int32_t* n_thin_dev,
                               int32_t* n_unsure_dev, void* stream);

/* ---- bone length and direction errors (`--eval_bones`) -------------------------------------------------------------------------
 * The points-based reports say how far the joints are; these two calls say what the SKELETON is: how long its bones are and where
 * they point.  No reference code pins the definition, so this text is the specification (tests/bone_cases.py restates it).
 * Joints in the order of the evaluation report (Pelvis, R_Hip, R_Knee, R_Ankle, L_Hip, L_Knee, L_Ankle, Torso, Neck, Nose, Head,
 * L_Shoulder, L_Elbow, L_Wrist, R_Shoulder, R_Elbow, R_Wrist); the parent of joint j is
 *   parent = { -1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15 }
 * and bone b = 1 .. 16 joins joint b to parent[b].  The six (left, right) pairs of bones are (4,1), (5,2), (6,3), (11,14), (12,15),
 * (13,16): pelvis-hip, thigh, shin, neck-shoulder, upper arm, forearm.
 * Per pose, with pred P (17,3) in metres and target G (17,3) in millimetres, as jrr_evaluate_joints takes them:
 *   x = P - P[0],  q = G / 1000.f,  y = q - q[0]                                  (both centred on the pelvis)
 *   u_b = x_b - x_parent,  v_b = y_b - y_parent
 *   |w| = sqrtf((w0 w0 + w1 w1) + w2 w2),  a . b = (a0 b0 + a1 b1) + a2 b2,
 *   a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)
 *   len_pred_b = |u_b|,  len_gt_b = |v_b|
 *   ang_b      = atan2f(|u_b x v_b|, u_b . v_b)      radians in [0, pi]; this form and not acosf, so that small angles keep their digits
 *   ang_pa_b   = the same between R u_b and v_b, (R u)_r = (R[r][0] u0 + R[r][1] u1) + R[r][2] u2, with R the rotation of the similarity
 *                fit of x to y (csrc/procfit.h, its rank-2 / 1 / 0 rules included) from moments formed as jrr_evaluate_joints forms them:
 *                mu1 = (sum_i x_i) / 17 and mu2 likewise, i ascending; then per joint i ascending x1 = x_i - mu1, x2 = y_i - mu2,
 *                var1 += x1[c] x1[c] for c = 0, 1, 2, and K[r][c] += x1[r] x2[c], r outer.  Scale and translation do not enter a direction.
 *                Where pred or target lie on a line the rotation about that line is free, and so is ang_pa.
 *   direction-only skeleton (the predicted directions with the true lengths):
 *                xd_0 = 0,  xd_b = xd_parent + u_b * (len_gt_b / len_pred_b),  e_dir_j = |xd_j - y_j|,  e_dir_0 = 0
 *   length-only skeleton (the true directions with the predicted lengths):
 *                xl_0 = 0,  xl_b = xl_parent + v_b * (len_pred_b / len_gt_b),  e_len_j = |xl_j - y_j|,  e_len_0 = 0
 * Every operation is rounded once in fp32 in the order written, nothing is fused into a sum.  A bone of length 0 in either skeleton
 * gives 0 / 0 = NaN along its chain, a NaN input NaN where it enters; neither disturbs another pose.
 *
 * jrr_bone_error writes vals_dev (batch, JRR_BONE_VALS) fp32, layout above.  One pose per thread, no value crosses lanes: a pose's 98
 * values do not depend on the batch, its neighbours or the launch.  batch == 0 returns JRR_OK without a launch.  JRR_ERR_ARG with a
 * message, and no launch: a NULL input, vals_dev NULL (there is no other output), batch < 0, a pointer that is not 4-byte aligned.
 * No engine is touched.                                                                                                        */
int jrr_bone_error(const float* pred_j3d_dev, const float* target_j3d_mm_dev, int batch, float* vals_dev, void* stream);
/* jrr_bone_accumulate ADDS the poses of vals_dev (batch, JRR_BONE_VALS), as jrr_bone_error wrote them, to rows group_dev[b] of
 * acc_dev: int64 [n_groups][JRR_BONE_ACC_ROW] + JRR_BONE_ACC_TRAILER words, layout above; the caller zeroes it once per report.
 * group_dev NULL: every pose in group 0.  1 <= n_groups <= JRR_EVAL_ACC_MAX_GROUPS.  A pose adds to exactly one class of words:
 *   group < 0: trailer word 0 only;  group >= n_groups: trailer word 1 only;
 *   one of its 98 values fails v < 1.0e3f (NaN, inf -- hence a bone of length 0 in either skeleton, a constant pred -- or absurd;
 *   the project's overflow cap, no tolerance): BAD += 1 only;
 *   otherwise COUNT += 1 and, with fixed24(v) = llrintf(v * 2^24), per bone b: SUM_LEN_PRED += fixed24(len_pred), SUM_LEN_GT +=
 *   fixed24(len_gt), SUM_ABS_DLEN += fixed24(fabsf(len_pred - len_gt)), SUM_ANG += fixed24(ang), SUM_ANG_PA += fixed24(ang_pa),
 *   SUM_SQ_PRED += q * q and SUM_Q_PRED += q with q = llrintf(len_pred * 65536.f), SUM_SQ_GT and SUM_Q_GT likewise (exact integers: the
 *   variance of the lengths from them, (n SUM_SQ - SUM_Q^2) / n^2, is exact whatever the order); per joint j: SUM_ERR_DIR += fixed24(e_dir), SUM_ERR_LEN += fixed24(e_len); per pair (l, r):
 *   SUM_ASYM_PRED += fixed24(fabsf(len_pred_l - len_pred_r)), SUM_ASYM_GT likewise.
 * Integer atomics only: the table is a function of the multiset of (pose, group) pairs -- not of the order, the split into calls or
 * the sharding over ranks (sum the ranks' tables).  batch == 0 returns JRR_OK without a launch; JRR_ERR_ARG with a message for a NULL
 * vals_dev or acc_dev, batch < 0, n_groups out of range, vals_dev / group_dev not 4-byte or acc_dev not 8-byte aligned.            */
int jrr_bone_accumulate(const float* vals_dev, const int32_t* group_dev, int batch, int n_groups, int64_t* acc_dev, void* stream);

/* ---- placing a posed body in the real camera (`--place_refined`) -----------------------------------
 * jrr_place_translation: per pose the translation t (SMPL `transl`: camera-frame point = model point + t) that brings the 17 joints
 * S_j (joints_dev (B,17,3) fp32, metres, as jrr_find_joints_forward returns them) onto their pixels (u_j, v_j) (j2d_dev (B,17,2)
 * fp32, full-frame pixels) under the pinhole camera fx = K[0][0], fy = K[1][1], cx = K[0][2], cy = K[1][2] of K_dev (B,3,3) fp32 (no
 * other entry is read).  weight_dev (B,17) fp32 or NULL (all ones): joint j TAKES PART when its weight is finite and > 0.  The
 * arithmetic is fp64 on the fp32 inputs, every operation rounded once in the order written (no contraction), sums over j ascending:
 *   linear start   with a = u - cx, b = v - cy every taking-part joint gives the rows (fx, 0, -a | a Z - fx X) and (0, fy, -b | b Z - fy Y)
 *                  of a system in t; A = sum w row row^T (the six entries of the upper triangle), y = sum w row rhs; t_lin solves
 *                  A t = y by the root-free Cholesky factorisation A = L D L^T: d0 = A00, l10 = A01 / d0, l20 = A02 / d0,
 *                  d1 = A11 - l10 A01, l21 = (A12 - l20 A01) / d1, d2 = (A22 - l20 A02) - l21 (A12 - l20 A01); z0 = y0,
 *                  z1 = y1 - l10 z0, z2 = (y2 - l20 z0) - l21 z1; t2 = z2 / d2, t1 = z1 / d1 - l21 t2, t0 = (z0 / d0 - l10 t1) - l20 t2.
 *                  A pivot d that fails d > 0 sets bit 1.
 *   cost           c(t) = sum_j w_j (ru^2 + rv^2), ru = fx (X + t0) / (Z + t2) + cx - u, rv likewise
 *   LM step        exactly n_iters of them, lambda = 1e-3 at first: with q = 1 / (Z + t2) the Jacobian rows (fx q, 0, -fx (X + t0) q q)
 *                  and (0, fy q, -fy (Y + t1) q q); H = sum w row row^T, g = sum w row r; (H + lambda diag(H)) d = -g by the same
 *                  factorisation (a failed pivot: bit 3, the step is rejected); t + d is accepted when c(t + d) < c(t) and every
 *                  taking-part joint keeps Z + t2 > 0 -- then lambda = max(lambda / 10, 1e-7) -- otherwise lambda = min(10 lambda, 1e7)
 *   errors         err_lin_j / err_j = sqrt(ru^2 + rv^2) at t_lin / at the result, for all 17 joints, rounded to fp32
 * trans_dev (B,3) DOUBLE, err_lin_dev (B,17) fp32 or NULL, err_dev (B,17) fp32, status_dev (B) int32 (JRR_PLACE_* bits above; bit 0:
 * fewer than 2 taking-part joints, or one of the pose's 51 + 34 coordinates or of its fx, fy, cx, cy is not finite -- a weight that is
 * not finite only keeps its joint out; bit 2: t_lin leaves a taking-part joint at Z + t2 <= 0).  A pose with bit 0, 1 or 2 holds NaN in
 * trans and in both error rows.  One pose per thread, staged through LDS; a pose's result depends on nothing but that pose -- not on
 * the batch, its position in it or the launch.  0 <= n_iters <= JRR_PLACE_MAX_ITERS.  batch == 0 returns JRR_OK without a launch;
 * JRR_ERR_ARG with a message, and no launch: a NULL joints_dev, j2d_dev, K_dev, trans_dev, err_dev or status_dev, batch < 0, n_iters
 * out of range, trans_dev not 8-byte or another array not 4-byte aligned.                                                        */
int jrr_place_translation(const float* joints_dev, const float* j2d_dev, const float* K_dev, const float* weight_dev, int batch, int n_iters,
                          double* trans_dev, float* err_lin_dev, float* err_dev, int32_t* status_dev, void* stream);
/* jrr_project_points: the pinhole projection itself, for the 17 joints and the 6890 vertices alike.  points_dev (B,N,3) fp32,
 * trans_dev (B,3) double -- rounded to fp32 once --, K_dev (B,3,3) as above; in fp32, each operation rounded once:
 *   d = Z + tz,  u = (fx * (X + tx)) / d + cx,  v = (fy * (Y + ty)) / d + cy
 * -> uv_dev (B,N,2) fp32, NaN for a point with d <= 0 (or d NaN), and depth_dev (B,N) fp32 or NULL: d itself.  batch == 0 or
 * n_points == 0 returns JRR_OK without a launch; JRR_ERR_ARG with a message: a NULL points_dev, trans_dev, K_dev or uv_dev, batch < 0,
 * n_points < 0, batch * n_points >= 2^31, trans_dev not 8-byte or another array not 4-byte aligned.                                */
int jrr_project_points(const float* points_dev, const double* trans_dev, const float* K_dev, int batch, int n_points, float* uv_dev,
                       float* depth_dev, void* stream);
/* jrr_place_accumulate ADDS the poses jrr_place_translation wrote to rows group_dev[b] of acc_dev: int64 [n_groups][JRR_PLACE_ACC_ROW]
 * + JRR_PLACE_ACC_TRAILER words, layout above; the caller zeroes it once per report.  group_dev NULL: every pose in group 0;
 * weight_dev NULL: every joint takes part; err_lin_dev NULL: the SUM_ERR_LIN words stay as they are.  A pose adds to exactly one class
 * of words:  group < 0: trailer word 0 only;  group >= n_groups: trailer word 1 only;  a status bit 0 .. 2, a trans_z that fails
 * |(float)trans_z| < 1.0e3f or an err / err_lin of a taking-part joint that fails e < 1.0e3f: BAD += 1 only;  otherwise COUNT += 1,
 * STEP_PIVOT += 1 with status bit 3, SUM_TZ += fixed24((float)trans_z) and per taking-part joint j JOINTS[j] += 1, SUM_ERR_LIN[j] +=
 * fixed24(err_lin_j), SUM_ERR[j] += fixed24(err_j), fixed24(v) = llrintf(v * 2^24).  Integer atomics only: the table is a function of
 * the multiset of poses -- not of the order, the split into calls or the sharding over ranks.  batch == 0 returns JRR_OK without a
 * launch; JRR_ERR_ARG with a message for a NULL trans_dev, err_dev, status_dev or acc_dev, batch < 0, n_groups out of range, trans_dev
 * or acc_dev not 8-byte or another array not 4-byte aligned.                                                                       */
int jrr_place_accumulate(const double* trans_dev, const float* err_lin_dev, const float* err_dev, const float* weight_dev,
                         const int32_t* status_dev, const int32_t* group_dev, int batch, int n_groups, int64_t* acc_dev, void* stream);

/* ---- what the real camera sees of a placed body (`--visible_refined`) ------------------------------
 * jrr_point_visibility: verts_cam_dev (B,n_verts,3) fp32, camera-frame metres (the caller has added the translation), with the
 * triangles faces_dev (n_faces,3) int32 the poses share.  The queries are points_cam_dev (B,n_points,3) fp32, or -- NULL, and then
 * n_points == n_verts -- the pose's own vertices, and for query i every face that names vertex i is skipped.  For a query p with depth
 * d = p_z and a face with corners a, b, c: the ray from the camera centre 0 to p meets the face's plane at s p, with barycentrics
 * lambda0, lambda1, lambda2 that sum to 1; the face CROSSES IN FRONT when min lambda >= 0, s > 0 and s d < d - margin_m.
 *   count   the number of such faces.  A face adds nothing when a corner is not finite, when (b - a) x (c - a) is zero in fp32, or
 *           when its plane passes through the camera centre.  A face with an index outside [0, n_verts) adds nothing and sets bit 0
 *           (JRR_DEPTH_STATUS_INDEX) of status_dev[0], which the caller zeroes; the other faces are counted.
 *   code    bit 0 (JRR_VIS_OCCLUDED): count >= min_crossings (1 for a vertex; 2 for an interior point such as a regressed joint,
 *           whose first crossing is its own skin);
 *           bit 1 (JRR_VIS_OUTSIDE): K_dev (B,3,3) and rect_dev (B,4) = [x0,y0,x1,y1] pixels are given (both or neither) and
 *           x0 <= u < x1, y0 <= v < y1 fails for the pixel u = (fx * X) / d + cx, v = (fy * Y) / d + cy of jrr_project_points: fp32,
 *           each operation rounded once, no contraction -- bit-exact against a float32 restatement; a NaN in K or rect fails it;
 *           bit 2 (JRR_VIS_INVALID): d <= 0 or a coordinate of p is not finite; count is then 0 and bits 0 and 1 stay clear.
 * The intersection is done in 3-D in fp32 on differences (Moeller-Trumbore with origin 0: e1 = b - a, e2 = c - a, h = p x e2,
 * det = e1 . h, lambda1 det = -(a . h), q = e1 x a, lambda2 det = p . q, s det = e2 . q; signs are compared against det, nothing is
 * divided), so a face that straddles Z = 0 is no special case.  A pair closer than about 3e-4 to an edge in a barycentric, or than
 * fp32 rounding of the depths to the margin, may fall either way; everywhere else count is the exact one.  One query per lane,
 * integer counts, no cross-lane step: a query's result depends on its pose alone -- not on the batch, its column or the launch.
 * count_dev (B,n_points) int32 or NULL, code_dev (B,n_points) uint8.  batch == 0 or n_points == 0 returns JRR_OK without a launch;
 * JRR_ERR_ARG with a message, no launch and nothing written: a NULL verts_cam_dev, faces_dev, code_dev or status_dev, batch < 0,
 * n_verts < 1, n_faces < 0, n_points < 0 or > JRR_VIS_MAX_POINTS, points NULL with n_points != n_verts, one of K_dev / rect_dev
 * without the other, an array other than code_dev not 4-byte aligned, margin_m not finite or < 0, min_crossings outside 1 .. 255.  */
int jrr_point_visibility(const float* verts_cam_dev, int batch, int n_verts, const int32_t* faces_dev, int n_faces, const float* points_cam_dev,
                         int n_points, const float* K_dev, const float* rect_dev, float margin_m, int min_crossings, int32_t* count_dev,
                         uint8_t* code_dev, int32_t* status_dev, void* stream);
/* jrr_visibility_accumulate ADDS the poses to rows group_dev[b] of acc_dev: int64 [n_groups][JRR_VIS_ACC_ROW] + JRR_VIS_ACC_TRAILER
 * words, layout above; the caller zeroes it once per report.  vert_code_dev (B,n_verts) and joint_code_dev (B,17) uint8 as
 * jrr_point_visibility wrote them; err_j_dev (B,17) fp32 mm or NULL (the SUM_ERR words stay as they are); part_dev (n_verts) int32 or
 * NULL (every vertex in part 0); pose_status_dev (B) int32 or NULL: the status of jrr_place_translation; group_dev NULL: every pose in
 * group 0; per_vertex_dev (n_verts) int64 or NULL.  A pose adds to exactly one class of words:  group < 0: trailer word 0 only;
 * group >= n_groups: trailer word 1 only;  BAD += 1 only, when its pose_status has one of the bits JRR_PLACE_BAD_BITS, when one of
 * its n_verts + 17 codes has a bit other than bits 0 and 1 set, or when one of its 17 errors fails e < 1.0e5f (NaN, infinite,
 * absurd);  otherwise COUNT += 1, the three SUM_VERT words, per joint J_SEEN / J_OCCLUDED / J_OUTSIDE and SUM_ERR_SEEN /
 * SUM_ERR_OCCLUDED += fixed24(err_j) = llrintf(err_j * 2^24), PART_ALL[part[v]] += 1 for every vertex and PART_SEEN[part[v]] += 1
 * and per_vertex_dev[v] += 1 for every vertex with code 0.  Integer atomics only: the tables are a function of the multiset of poses
 * -- not of the order, the split into calls or the sharding over ranks.  batch == 0 returns JRR_OK without a launch; JRR_ERR_ARG with
 * a message for a NULL vert_code_dev, joint_code_dev or acc_dev, batch < 0, n_groups out of range, n_verts outside
 * 1 .. JRR_VIS_MAX_POINTS, acc_dev or per_vertex_dev not 8-byte or another int32 / fp32 array not 4-byte aligned.                    */
int jrr_visibility_accumulate(const uint8_t* vert_code_dev, const uint8_t* joint_code_dev, const float* err_j_dev, const int32_t* part_dev,
                              const int32_t* pose_status_dev, const int32_t* group_dev, int batch, int n_verts, int n_groups, int64_t* acc_dev,
                              int64_t* per_vertex_dev, void* stream);

/* ---- 2-D reprojection --------------------------------------------
 * return_2d_joints core, scripts/renderer.py:35-49 (pytorch3d 0.3.0 PerspectiveCameras, R = I,
 * T = cam, focal 5000/224 NDC, 224x224): joints (B,17,3), cam (B,3) -> screen xy (B,17,2).       */
int jrr_project_joints(const float* joints_dev, const float* cam_dev, float* j2d_dev, int batch, void* stream);
/* Enable (gt_j2d_dev != NULL) / disable the 2-D term  mean((gt_j2d - joints_2d)^2)/100  of the inner
 * loop (scripts/optimize.py:231-233,252); the camera translation then joins the Adam parameters
 * (optimize.py:201-202): cam (B,3) in place, cam_m / cam_v (B,3) its Adam state.                   */
int jrr_engine_set_reprojection(jrr_engine_t* e, const float* gt_j2d_dev, float* cam_dev, float* cam_m_dev,
                                float* cam_v_dev);
/* Camera pre-fit, scripts/optimize.py:187-199: n_steps Adam(lr) steps on cam against the 2-D joints
 * of the current pose.  The joints do not depend on the camera, so SMPL runs ONCE and the n_steps
 * run inside one kernel.  sq2d_dev (B, nullable): squared 2-D error at the last evaluation.        */
int jrr_camera_prefit(jrr_engine_t* e, const float* x6d_dev, const float* betas_dev, const float* gt_j2d_dev,
                      float* cam_dev, int n_steps, float lr, float* sq2d_dev, void* stream);

/* ---- soft silhouette (BASELINE configs[4]) ---------------------------
 * render_mesh(...) = Mesh_Renderer(224)(batch, verts*[-2,-2,2])[:, 3], scripts/optimize.py:77-85 +
 * scripts/mesh_renderer.py:23-79 (pytorch3d 0.3.0 rasteriser, blur_radius 0, 1 face per pixel,
 * SoftSilhouetteShader sigma 1e-4).  verts (B,6890,3), cam (B,3) -> alpha (B,224,224).
 * Image size: 224 (JRR_SIL_SIZE: what the reference's loop instantiates, scripts/optimize.py:110 `Mesh_Renderer(image_size=224)`)
 * or -- engines created with JRR_FLAG_SIL_256 -- 256, the constructor's own default (scripts/mesh_renderer.py:25); the camera's focal
 * length is 5000 / size (mesh_renderer.py:52-53).  The kernels are instantiated for these two sizes (the pixel-index packing of the
 * covered-pixel lists holds 16 bits: at most 256 x 256); the host mirror's Mesh_Renderer raises NotImplementedError for others. */
int jrr_silhouette_forward(jrr_engine_t* e, const float* verts_dev, const float* cam_dev, float* alpha_dev,
                           void* stream);
/* adjoint for the SAME inputs (must follow the forward): galpha (B,224,224) -> dverts (B,6890,3), dcam (B,3);
 * float atomics: summation order (last bits) varies between runs.                                    */
int jrr_silhouette_backward(jrr_engine_t* e, const float* galpha_dev, float* dverts_dev, float* dcam_dev,
                            void* stream);
/* pix_to_face of the most recent rasterisation on this engine (jrr_silhouette_forward, jrr_silhouette_loss_grad or the
 * last silhouette iteration of jrr_refine_run): the pytorch3d rasteriser's Fragments.pix_to_face at faces_per_pixel = 1
 * (scripts/mesh_renderer.py:34-38,59-63): (B,224,224) int32, -1 = background, else the index of the nearest face.      */
int jrr_silhouette_pix_to_face(jrr_engine_t* e, int32_t* pix_to_face_dev, void* stream);
/* Enable (mask_dev != NULL, (B,224,224)) / disable the term 100 * mean((silhouette - mask)^2) of the inner
 * loop (scripts/optimize.py:234-237,252); shares the camera parameter with jrr_engine_set_reprojection.
 * The engine caches sum(mask^2) per pose at the next jrr_refine_run: call this again after changing the mask's contents. */
int jrr_engine_set_silhouette(jrr_engine_t* e, const float* mask_dev, float* cam_dev, float* cam_m_dev,
                              float* cam_v_dev);

/* The silhouette term as the fused inner loop evaluates it (projection from the engine's internal vertex layout, nearest
 * face per pixel, loss and adjoint in one kernel), exposed as an operator: SMPL forward of (x6d, betas), then
 * sqsil_dev[b] = sum_pixels (silhouette - mask)^2 and the gradient of 100 * mean((silhouette - mask)^2) (mean over
 * batch_norm * 224 * 224; scripts/optimize.py:234-237,252) w.r.t. the SMPL vertices, dverts_dev (B,6890,3), and the
 * camera, dcam_dev (B,3).  mask_dev (B,224,224).  Outputs nullable.  Needs JRR_FLAG_SILHOUETTE | JRR_FLAG_KEEP_VERTS.
 * Bitwise reproducible (fixed-point accumulation), unlike jrr_silhouette_backward.                                   */
int jrr_silhouette_loss_grad(jrr_engine_t* e, const float* x6d_dev, const float* betas_dev, const float* cam_dev,
                             const float* mask_dev, float* sqsil_dev, float* dverts_dev, float* dcam_dev, void* stream);

/* ---- fused inner loop ---------------------------------------------------------------------
 * n_iters iterations of scripts/optimize.py:220-265 restricted to the engine's loss terms:
 * rot6d->R, SMPL, J-regress, pelvis-centre, MSE x10000 [+ pose-D x10] [+ shape-D x10],
 * analytic backward to (pose6d, betas), Adam(lr) in place.  x6d (B,24,6) holds orient (joint 0)
 * and pose (joints 1..23); adam_m/adam_v (B,154) = [144 pose | 10 betas]; step_dev counts
 * completed Adam steps (0 before the first).  sqerr_dev (B) receives the per-pose squared
 * joint error of the LAST iteration's forward (may be NULL).                                  */
int jrr_refine_run(jrr_engine_t* e, float* x6d_dev, float* betas_dev, const float* gt_centred_mm_dev,
                   float* adam_m_dev, float* adam_v_dev, int32_t* step_dev, float lr, int n_iters,
                   float* sqerr_dev, void* stream);

/* Adversarial loss values of the LAST iteration of the last jrr_refine_run, for the reference's log record
 * (scripts/optimize.py:246-250,323-337 `pose_discriminated_loss`, `shape_discriminated_loss`):
 * pose_disc_sq_dev[b] = sum_k (D(x_b)[k] - 1)^2 over the 25 outputs, shape_disc_sq_dev[b] = (SD(beta_b) - 1)^2.
 * Either pointer may be NULL; a non-NULL one needs its term active in the engine.                           */
int jrr_refine_aux_losses(jrr_engine_t* e, float* pose_disc_sq_dev, float* shape_disc_sq_dev, void* stream);

/* J step, scripts/optimize.py:300-312: gradient of mean((move_pelvis(joints)-gt/1000)^2) w.r.t.
 * the raw J_regressor for the current (detached) poses; dJ_dev (17,6890).  sqerr_dev (B, nullable): per-pose squared
 * joint error; joints_dev (B,17,3, nullable): the joints of this forward, i.e. of the regressor BEFORE its step (what
 * utils.evaluate reads at scripts/optimize.py:314-315).  The product behind it runs over the POSITIVE entries of
 * J*mask only (dJ is exactly zero elsewhere: relu'); rows with more than 128 of them switch to the dense product by
 * themselves (device-side decision, no synchronisation).                                                         */
int jrr_j_regressor_grad(jrr_engine_t* e, const float* x6d_dev, const float* betas_dev,
                         const float* gt_centred_mm_dev, float* dJ_dev, float* sqerr_dev, float* joints_dev, void* stream);

/* The second half of the J step in one call: step_dev += 1, torch.optim.Adam(lr) on the raw regressor J_dev (17,6890)
 * in place with the (all-reduced) gradient dJ_dev and the state m_dev / v_dev, then J*mask -> ReLU -> row-normalise into
 * the engine's layouts (= jrr_adam_step + jrr_engine_set_j_regressor).  Under data parallelism the J step is
 * jrr_j_regressor_grad -> ONE RCCL all-reduce of dJ -> jrr_j_step_apply (scripts/optimize.py:300-312).  mask_dev nullable. */
int jrr_j_step_apply(jrr_engine_t* e, float* J_dev, const float* dJ_dev, float* m_dev, float* v_dev, int32_t* step_dev,
                     float lr, const float* mask_dev, void* stream);

/* The J step's all-reduce restricted to the regressor's SUPPORT (data parallelism; scripts/optimize.py:300-312 under sharding).
 * dJ w.r.t. the raw regressor is exactly zero wherever J*mask <= 0 (ReLU'), so the ranks only need to exchange its values on the
 * positive entries: [17][128] floats (8 704 bytes) instead of 17 x 6890 (468 520 bytes).  Every rank holds the same regressor,
 * hence the same device-side support lists (ascending vertex order).
 *   jrr_j_support_info            positive entries per row (counts_host[17], nullable) and fits_host = 1 when every row has at
 *                                 most 128 of them.  SYNCHRONOUS (waits for `stream`); call once after jrr_engine_set_j_regressor:
 *                                 J steps only ever shrink the support (an entry at <= 0 gets no gradient), so the answer holds
 *                                 until the next jrr_engine_set_j_regressor from outside or a J step with ANOTHER mask pointer (a
 *                                 mask whose contents change in place must be re-announced through jrr_engine_set_j_regressor).
 *                                 Once the engine has been told that the
 *                                 support fits, EVERY J step on it (jrr_j_regressor_grad, jrr_refine_run_j_steps, the forward reuse)
 *                                 enqueues the support-restricted products only; before, the dense products are enqueued beside them
 *                                 and a device flag picks (no host knowledge needed, ~14 us of idle launches per J step).
 *   jrr_j_regressor_grad_support  = jrr_j_regressor_grad, gradient delivered as dJs_dev [17][128] (0 behind a row's count)
 *   jrr_j_step_apply_support      = jrr_j_step_apply with the (all-reduced) dJs_dev: the dense gradient is rebuilt on the device
 *                                 (zero outside the support, as the dense path has it) and torch's Adam runs over the whole
 *                                 (17,6890) parameter as before -- entries that left the support keep coasting on their momentum.
 *                                 Its forward (and that of the in-call steps of jrr_refine_run_j_steps) keeps the vertices of
 *                                 the 32-vertex tiles that hold a support entry only -- what the gradient product and the reusing
 *                                 iteration read -- not all 6890 x 3 x B of them: a jrr_find_joints_backward(dJ) afterwards
 *                                 needs its own jrr_find_joints_forward, and a jrr_engine_set_j_regressor from outside between
 *                                 this call and jrr_refine_run_after_j_step drops the cached forward (JRR_ERR_STATE there).
 * Both return JRR_ERR_STATE unless jrr_j_support_info has reported fits = 1 for the current regressor (fall back to the
 * dense pair).  Same results as the dense pair bit for bit on this rank; across ranks only the all-reduce's own summation
 * order can differ (none with two ranks).                                                                                  */
int jrr_j_support_info(jrr_engine_t* e, int32_t* counts_host, int32_t* fits_host, void* stream);
/* JRR_FLAG_SUPPORT_TILES: returns 1 when the next joint-loss iteration of jrr_refine_run* will run on the support's tiles only
 * (*n_tiles_host = their number, nullable), 0 when it will run all 216 (flag absent, jrr_j_support_info not asked or fits = 0,
 * a silhouette term set, folded mode on, a model without the joint-sparse kernels).  No reference counterpart: the reference
 * multiplies all 6890 vertices by the (17,6890) regressor, zeros included (scripts/utils.py:87-92).                          */
int jrr_engine_support_tiles(const jrr_engine_t* e, int32_t* n_tiles_host);
/* ... and returns 1 when those iterations run per support VERTEX (*n_vertices_host = the vertices the regressor reads, nullable): the
 * support then has at most 64 vertices and ONE launch per iteration takes a 32-pose group through chain forward, the SMPL forward
 * of the support vertices, the joint loss [+ the 2-D term] (scripts/utils.py:87-114, scripts/optimize.py:231-233), its backward, the
 * chain adjoint and Adam (scripts/optimize.py:220-265) -- preceded by the discriminator's four GEMM launches when it is on.  0: the tile lists above (or
 * all tiles) run as separate launches.  Same numbers up to the order of the sums.  JRR_SUPPORT_FUSED=0 in the environment of
 * jrr_j_support_info keeps the tile lists (verification).  No reference counterpart.                                              */
int jrr_engine_support_vertices(const jrr_engine_t* e, int32_t* n_vertices_host);
int jrr_j_regressor_grad_support(jrr_engine_t* e, const float* x6d_dev, const float* betas_dev, const float* gt_centred_mm_dev,
                                 float* dJs_dev, float* sqerr_dev, float* joints_dev, void* stream);
int jrr_j_step_apply_support(jrr_engine_t* e, float* J_dev, const float* dJs_dev, float* m_dev, float* v_dev, int32_t* step_dev,
                             float lr, const float* mask_dev, void* stream);

/* Forward reuse across the J step (needs JRR_FLAG_KEEP_VERTS).  jrr_j_regressor_grad evaluates SMPL on the current
 * poses; the inner iteration that follows evaluates it on the SAME poses (only the regressor has changed in between,
 * scripts/optimize.py:300-312 then :220-229).  jrr_refine_run_after_j_step is jrr_refine_run whose FIRST iteration
 * re-regresses its joints from the J step's stored vertices with the new regressor instead of repeating the forward --
 * the same arithmetic up to the summation order of the regressor product.  Reuse is explicit per call: by calling this
 * entry point the caller states that the previous calls on this engine were jrr_j_regressor_grad on the same x6d / betas
 * buffers (optionally followed by jrr_j_step_apply / jrr_engine_set_j_regressor) and that nothing has written those
 * buffers since.  What the engine can check it checks: the stored forward is dropped by every entry point that enqueues work
 * on the engine's workspace, uploads parameters or changes a loss term (jrr_find_joints_forward / _backward, jrr_smpl_*_backward, jrr_pose_disc_*,
 * jrr_shape_disc_*, jrr_silhouette_forward / _backward / _loss_grad, jrr_camera_prefit, jrr_refine_run, jrr_refine_aux_losses,
 * jrr_engine_set_folded / _pose_disc / _shape_disc / _reprojection / _silhouette), and by jrr_engine_set_j_regressor when the J
 * step stored the support's tiles only (jrr_j_step_apply_support above); the call then returns JRR_ERR_STATE (also when the
 * pointers differ) instead of differentiating through a stale forward.  It is kept by the J step's own calls, by
 * jrr_find_joints_after_j_step, and by the calls that only read or configure: jrr_smpl_posed_joints,
 * jrr_silhouette_pix_to_face, jrr_j_support_info (unless it reports a grown support), jrr_engine_support_tiles / _vertices,
 * jrr_engine_info, jrr_engine_set_batch_norm, the loss history, profiling and probe calls (tests/test_gpu_engine_state.py holds
 * every entry point to this list).                                                                                     */
int jrr_refine_run_after_j_step(jrr_engine_t* e, float* x6d_dev, float* betas_dev, const float* gt_centred_mm_dev,
                                float* adam_m_dev, float* adam_v_dev, int32_t* step_dev, float lr, int n_iters,
                                float* sqerr_dev, void* stream);

/* The inner loop WITH its J steps in one call, for a single process (no collective between the two halves of a J step):
 * n_iters iterations of jrr_refine_run; after every j_every-th one the J step of scripts/optimize.py:300-312
 * (jrr_j_regressor_grad into engine scratch, jrr_j_step_apply with J_dev / J_m_dev / J_v_dev / J_step_dev / j_lr /
 * mask_dev), the next iteration reusing its forward.  j_sqerr_dev (B, nullable): per-pose squared joint error of the
 * last J step.  after_j_step bit 0: as jrr_refine_run_after_j_step for the first iteration; bit 1 (value 2): NO forward reuse
 * inside the call either -- every iteration repeats its SMPL forward (the reference draws a new batch after each J step,
 * scripts/optimize.py:144-148, so nothing is shared there: what bench.py's headline times).  BASELINE configs[3]'s
 * "J_regressor step each iteration" at world size 1 is j_every = 1.  Needs JRR_FLAG_KEEP_VERTS.                       */
int jrr_refine_run_j_steps(jrr_engine_t* e, float* x6d_dev, float* betas_dev, const float* gt_centred_mm_dev,
                           float* adam_m_dev, float* adam_v_dev, int32_t* step_dev, float lr, int n_iters,
                           float* sqerr_dev, int j_every, float* J_dev, float* J_m_dev, float* J_v_dev,
                           int32_t* J_step_dev, float j_lr, const float* mask_dev, float* j_sqerr_dev, int after_j_step,
                           void* stream);

/* Loss history of the inner loop (scripts/optimize.py:255-261 prints the five weighted terms when i % 10 == 0): while
 * hist_dev != NULL, every `every`-th iteration run by jrr_refine_run* (counted from this call, first one included)
 * appends one record of 5 floats {loss_j2d/100, silhouette_loss*100, joint_loss*10000, pose_discriminated_loss*10,
 * shape_discriminated_loss*10} (inactive terms 0) to hist_dev, up to capacity_records.  Each value is this engine's
 * share of the global mean (local sum / batch_norm denominators): under data parallelism the ranks' records add up.
 * jrr_engine_loss_history_count returns the number of records written so far.  hist_dev == NULL disables.            */
int jrr_engine_set_loss_history(jrr_engine_t* e, float* hist_dev, int capacity_records, int every);
int jrr_engine_loss_history_count(const jrr_engine_t* e);

/* launch geometry: {B, BP, batch_norm, nvc, nvcb, nsplit, nsplitJ, flags, joint_sparse}; joint_sparse = 8 or 12: the LBS kernels
 * multiply each 32-vertex tile by its own joints only, that many slots per pass (exact: the skipped terms are zeros; a tile with
 * more joints runs a second pass, jrr_model_info), 0 = dense kernels (a tile with more than 16 joints, or JRR_DENSE_SKINNING=1 in
 * the environment of jrr_model_create) */
int jrr_engine_info(const jrr_engine_t* e, int32_t* out, int n);

/* Per-kernel timing of jrr_refine_run with HIP events recorded on the launch stream.
 * While enabled, every launch group of every iteration is bracketed by an event pair.
 * jrr_engine_profile_read synchronises on the recorded events and writes the MEAN duration in
 * milliseconds per launch of each class into ms_host[JRR_PROF_CLASSES] and the number of samples
 * into counts_host, then clears the recorded events.  Classes:
 *   0 chain forward (+ the pose discriminator's per-joint MLP, same launch)  1 k_lbs_fwd  2 k_joints_loss  3 k_lbs_bwd
 *   4 blend adjoint  5 pose discriminator: the four wide-layer products  6 k_shape_disc
 *   7 dF slab sum (+ per-joint MLP adjoint, same launch) and k_chain_bwd (+Adam)  8 silhouette (fwd+bwd) */
enum { JRR_PROF_CLASSES = 9 };
int jrr_engine_set_profiling(jrr_engine_t* e, int enabled);
int jrr_engine_profile_read(jrr_engine_t* e, float* ms_host, int32_t* counts_host);
/* Shader-clock probe of the dominant kernel (k_lbs_fwd), recorded while profiling is on by workgroup 0 / wave 0
 * of the last launch inside jrr_refine_run: out[0] = shader clocks the wave was resident (s_memtime),
 * out[1] = MFMA instructions it issued, out[2] = waves resident per SIMD, out[3] = issue clocks per MFMA,
 * out[4] = the same interval in ns (s_memrealtime).  MFMA-pipe occupancy = out[1]*out[2]*out[3]/out[0];
 * sustained shader clock = out[0]/out[4] GHz.  out_host holds 5 values.  Synchronous (device -> host copy).
 * (48 of the 423 instructions per tile of the joint-sparse kernel are the 33-clock four-block form v_mfma_f32_16x16x1_4b_f32:
 * the occupancy formula, which prices every instruction at out[3] = 64 clocks, reads ~5 % high for it.)               */
int jrr_engine_probe_read(jrr_engine_t* e, int64_t* out_host);

/* The regressor fit (`--fit_regressor`): Adam steps of the J_regressor on a table of FIXED meshes, scripts/optimize.py:300-312 with
 * the SMPL forward taken out of the loop.  ReLU' zeroes the gradient outside the positive entries of J*mask, and an entry whose
 * gradient is always zero keeps m = v = 0 under torch.optim.Adam and never moves: a step needs, per sample, the vertices of those
 * entries and the ground truth.  No engine, no body model.
 *
 * STATE (state_dev: caller-owned, 16-byte aligned, jrr_jfit_state_bytes bytes; opaque).  jrr_jfit_prepare builds it from J_init_dev
 * (17,6890) raw and mask_dev (17,6890) or NULL:
 *   cols[NS]   the union of the columns where J_init*mask > 0 in any row, ascending vertex index, 1 <= NS <= 17 * 128;
 *   per row i  the list of its positive entries in ascending vertex order, at most JRR_JFIT_ROW_CAP = 128 of them: each entry's
 *              position in cols, its raw value, its mask value, Adam's m = v = 0; the Adam step counter 0.
 * A row with more than 128 positive entries, or no positive entry in any row: JRR_ERR_ARG.  A row without a positive entry is
 * accepted: it has no parameters and stays as it is; jrr_jfit_joints gives NaN for its joint (the reference's 0/0), and jrr_jfit_run
 * leaves that joint out of the loss and of the adjoint (the mean still divides by count * 17 * 3; an empty PELVIS row centres the
 * other joints on the origin) instead of letting the NaN reach every other row through the centring.  The call synchronises the
 * stream and fills info_host[JRR_JFIT_INFO] (nullable): {NS, listed entries, Adam steps taken, 0, entries of row 0 .. 16}.
 * jrr_jfit_info reads the same words of a prepared state back (synchronises).
 *
 * CACHE (cache_dev: caller-owned, 16-byte aligned, jrr_jfit_cache_bytes(n_rows, ns) bytes).  Sample-major rows of
 *   RL = (3 ns + 51) | 1 floats:  [0, 3 ns) the support vertices, x y z of cols[0], cols[1], ...;  [3 ns, 3 ns + 51) the ground truth
 *   (17,3), pelvis-centred, in mm;  one float of padding (zero) when 3 ns + 51 is even.
 * Row r starts at float r * RL: a minibatch of consecutive rows is ONE contiguous run of bytes, which the step kernel streams into
 * LDS with coalesced loads, and a row permutation is an index copy of a (n_rows, RL) fp32 array (the odd stride keeps the samples of
 * a workgroup on different LDS banks).  `ns` of every call must be the prepared NS: a mismatch found on the device sets the error
 * word of the state (the one thing gather and joints write there: their state pointer is not const) that the next jrr_jfit_info
 * reports as JRR_ERR_ARG, and the launch writes nothing but NaN losses / NaN joints.
 *
 * jrr_jfit_gather  verts_dev (batch,6890,3), gt_mm_dev (batch,17,3) -> cache rows [row0, row0 + batch).
 * jrr_jfit_joints  joints_dev (count,17,3) of cache rows [begin, begin + count) under the CURRENT entries: x = relu(raw * mask),
 *                  Jn = x / rowsum(x), joints = Jn @ verts; NOT pelvis-centred; each sum in double, in list order, one rounding.
 * jrr_jfit_run     n_steps consecutive Adam steps, all enqueued without a host synchronisation; step k uses cache rows
 *                  [(first + k) * batch, min((first + k + 1) * batch, n_rows)); 0 <= first, first + n_steps <= ceil(n_rows / batch)
 *                  (else JRR_ERR_ARG; n_steps = 0 does nothing).  One step: joints as above, minus joint 0;
 *                  loss = mean over count * 17 * 3 of (joints - gt / 1000)^2 -> loss_dev[k] (the loss BEFORE the update); backward
 *                  through the centring (joint 0 receives minus the sum of all joint adjoints) and the normalisation,
 *                  mask * relu'(raw * mask) * (dJn - sum(dJn * Jn)) / rowsum; torch.optim.Adam(lr) on EVERY listed entry (one that has
 *                  gone non-positive coasts on its moments).  A short last minibatch divides by its own count.  grad_dev (nullable)
 *                  [17][128] receives the gradient of the LAST step with respect to the raw entries, entry e of row i at
 *                  i * 128 + e, zeros behind a row's count.  ONE launch per step: workgroup w of min(ceil(count / JRR_JFIT_SPW),
 *                  JRR_JFIT_MAX_WG) sums the samples of its 32-sample chunks w, w + grid, ... in double into a slab of the state;
 *                  the workgroup that arrives last (integer atomic counter) adds the slabs in workgroup order and updates.  No
 *                  floating-point atomics: results are bitwise reproducible.
 * jrr_jfit_scatter the listed entries' raw values, m and v into dense (17,6890) arrays (each nullable); other elements are not
 *                  written: the caller fills them with J_init and zeros.                                                      */
enum { JRR_JFIT_ROW_CAP = 128, JRR_JFIT_SPW = 32, JRR_JFIT_MAX_WG = 256, JRR_JFIT_INFO = 24 };
size_t jrr_jfit_state_bytes(void);
size_t jrr_jfit_cache_bytes(int64_t n_rows, int ns);
int jrr_jfit_prepare(const float* J_init_dev, const float* mask_dev, void* state_dev, size_t state_bytes, int32_t* info_host,
                     void* stream);
int jrr_jfit_info(const void* state_dev, int32_t* info_host, void* stream);
int jrr_jfit_gather(void* state_dev, const float* verts_dev, const float* gt_mm_dev, int batch, void* cache_dev, int64_t n_rows,
                    int64_t row0, int ns, void* stream);
int jrr_jfit_joints(void* state_dev, const void* cache_dev, int64_t n_rows, int64_t begin, int count, int ns, float* joints_dev,
                    void* stream);
int jrr_jfit_run(void* state_dev, const void* cache_dev, int64_t n_rows, int ns, int batch, int64_t first, int n_steps, float lr,
                 float* loss_dev, float* grad_dev, void* stream);
int jrr_jfit_scatter(const void* state_dev, float* J_dev, float* m_dev, float* v_dev, void* stream);

/* The exact solve of the regressor fit (`--fit_solve`): with the meshes fixed, the loss of jrr_jfit_run is a convex quadratic in the
 * normalised weights, and its data enter only through the second moments of the cache rows.  Two entry points on the state and the
 * cache above; the solver itself runs on the host (regressor_solve.py).
 *
 * MOMENTS.  A cache row is W = ns + 17 points of 3 floats: the ns support vertices (m), then the 17 pelvis-centred ground-truth
 * joints (mm).  For cache rows [begin, begin + count)
 *     M[w][w'] = sum over the rows and the axes c < 3 of row[3 w + c] * row[3 w' + c]            (W x W doubles, row-major, symmetric)
 * with the blocks G = M[:ns,:ns] (m^2), C = M[ns:,:ns] (mm m) and the diagonal of M[ns:,ns:] (mm^2: its sum is sum gt^2).  Every
 * product of two fp32 values is formed exactly in fp64 and summed in fp64 (v_mfma_f64_16x16x4_f64; an fp32 Gram would round G by
 * more than the optimality gap the solve certifies: the loss is about 1e-4 of the scale of G).  The rows are cut into equal chunks of
 * at most JRR_JFIT_MOM_CHUNK rows, or longer ones where that would take more than JRR_JFIT_MOM_MAX_CHUNKS (fewer for a wide support: the chunks' partial sums, one
 * slab of doubles each, must fit the scratch); a second launch adds the slabs in a fixed order (four consecutive quarters of the
 * chunks, each in chunk order, then the quarters) and writes both triangles of M from the same sum.  No floating-point atomics: two calls give the same bits and M equals its transpose bitwise.
 *
 * jrr_jfit_moments_bytes  the bytes of M (W * W * 8) for this ns; *scratch_bytes (nullable) receives the bytes of the caller-owned
 *                  scratch, a function of ns alone.  ns outside 1 .. 2176: both 0.
 * jrr_jfit_moments  M_dev (8-byte aligned, jrr_jfit_moments_bytes bytes) of cache rows [begin, begin + count); count == 0 zeroes M.
 *                  scratch_dev: 8-byte aligned, scratch_bytes of it; nothing is kept there between calls.  NULL pointers,
 *                  misalignment, a range outside [0, n_rows] or an ns outside 1 .. 2176: JRR_ERR_ARG; a scratch below
 *                  jrr_jfit_moments_bytes: JRR_ERR_WORKSPACE.  An ns that is not the prepared NS is found on the device: the error
 *                  word of the state is set as by gather / joints (the next jrr_jfit_info reports it) and M is filled with NaN.
 *                  Enqueued on the stream, nothing is read back.
 * jrr_jfit_set_entries  loads the raw value of every LISTED entry from the dense J_dev (17,6890); zeros and negative values are
 *                  allowed and elements outside the lists are not read.  Adam's m and v of every entry and the step counter are
 *                  reset to 0, and the normalised weights and row sums are recomputed as a step leaves them (relu(raw * mask) over
 *                  its row sum, the sum in double).  A listed row whose relu(raw * mask) sums to 0 (or is not finite) sets the
 *                  error word, which the next jrr_jfit_info reports as JRR_ERR_ARG until a later jrr_jfit_set_entries leaves no
 *                  such row; its weights are NaN.  It is how the solved weights reach jrr_jfit_joints / jrr_evaluate, and how a
 *                  state prepared from a pattern of candidate entries (ones on the pattern) receives the true initial values: a
 *                  listed entry at zero has relu' = 0 and does not move under jrr_jfit_run.                                      */
enum { JRR_JFIT_MOM_CHUNK = 64, JRR_JFIT_MOM_MAX_CHUNKS = 1024 };
size_t jrr_jfit_moments_bytes(int ns, size_t* scratch_bytes);
int jrr_jfit_moments(void* state_dev, const void* cache_dev, int64_t n_rows, int64_t begin, int64_t count, int ns, double* M_dev,
                     void* scratch_dev, size_t scratch_bytes, void* stream);
int jrr_jfit_set_entries(void* state_dev, const float* J_dev, void* stream);

/* The MPJPE solve of the regressor fit (`--fit_solve --fit_solve_loss mpjpe`): every figure the project reports for a regressor is the
 * mean Euclidean distance per joint, and with the meshes fixed that is a convex function of the normalised weights too -- a mean of
 * norms of affine maps -- on the same product of simplices.  One entry point on the state and the cache above gives, per pass, the
 * objective, its exact gradient and the quadratic majoriser the host minimises (regressor_solve.py, solve_norm).
 *
 * Per cache row s and joint i = 1 .. 16 whose row has entries (x: the caller's weights, v: the row's support vertices):
 *     q_i = sum_e x_i[e] v[col_i[e]],  q_0 likewise (0 when the pelvis row is empty)
 *     r   = q_i - q_0 - gt_i / 1000                      3 doubles, m; everything in double from the fp32 cache values
 *     rho = sqrt(r.r + delta^2), delta > 0               L_delta(x) = sum_{s,i} rho / (n 17)
 *     L(x) = sum |r| / (n 17)                            1000 L is the training MPJPE in mm: the pelvis term is zero and the mean still
 *                                                        divides by 17, as jrr_evaluate does;  L <= L_delta <= L + delta.
 * A row without entries is left out of the sums, exactly as jrr_jfit_run leaves it out.  L_delta is smooth and convex; on the product of
 * simplices 0 <= L_delta(x) - min L_delta <= gap(x), the Frank-Wolfe gap with the gradient of L_delta, hence L(x) - min L <= gap(x) + delta.
 * Majoriser at x^k:  rho(r) <= rho_k + (|r|^2 - |r_k|^2) / (2 rho_k).  The points p_a of joint i are the vertices of row i's entries in
 * list order, then those of row 0's entries in list order: K_i = cnt_i + cnt_0 <= 256.  With D_i = (x_i - x_i^k ; -(x_0 - x_0^k)),
 *     Q(x) = L_delta(x^k) + (1 / (n 17)) sum_i [ b_i . D_i + 1/2 D_i^T A_i D_i ]
 *     A_i[a][b] = sum_s w sum_c p_a,c p_b,c      b_i[a] = sum_s w sum_c r_c p_a,c      w = 1 / rho_k
 * and any x with Q(x) <= Q(x^k) has L_delta(x) <= L_delta(x^k).  b_i is also the exact gradient of (n 17) L_delta at x^k (the pelvis row
 * collects minus each joint's second half).  Forming r directly in double avoids the cancellation that forced fp64 on jrr_jfit_moments.
 *
 * jrr_jfit_norm_bytes   the bytes of the output for the rows' counts (counts[17], as jrr_jfit_info reports them); *scratch_bytes
 *                  (nullable) receives the bytes of the caller-owned scratch.  Both are functions of the counts alone; a count outside
 *                  0 .. 128 or a NULL counts: both 0.
 * jrr_jfit_norm_moments  of cache rows [begin, begin + count).  The state supplies only the LISTS (each row's entries and counts); the
 *                  weights are x_dev [17][128] doubles, entry e of row i at i * 128 + e (entries behind a row's count are not read): the
 *                  certificate is about exactly the point the host holds, not about the state's fp32 copy of it.
 *                  out_dev holds, for i = 1 .. 16 in order, a block of K_i^2 + K_i + 4 doubles: A_i row-major, b_i, then
 *                  sum rho, sum |r|, sum w and the number of samples counted.  K_i = 0 when row i is empty: only the four scalars,
 *                  zeros.  JRR_JFIT_NORM_UNIT: w = 1 and delta_m >= 0 enters rho alone (rho = sqrt(r.r + delta^2), which is |r| at
 *                  delta = 0); A_i is then the gathered sub-block of jrr_jfit_moments' M and the quadratic is the `--fit_solve`
 *                  problem.  JRR_JFIT_NORM_INV: w = 1 / rho, and delta_m must be finite and > 0.
 *                  The rows are cut into chunks as by jrr_jfit_moments; a second launch adds the chunks' slabs in a fixed order and
 *                  writes both triangles of A_i from the same sum.  No floating-point atomics: two calls give the same bits,
 *                  A_i == A_i^T bitwise, count == 0 zeroes the output.  The call reads the 17 counts of the state back before it
 *                  launches (it synchronises the stream once); the results are enqueued, not read back.
 *                  NULL pointers, misalignment (state and cache 16 bytes; x, out, scratch 8), a range outside [0, n_rows], an ns
 *                  outside 1 .. 2176, an unknown mode, a delta_m that is negative or not finite, or not positive in INV mode, a state
 *                  that is not a prepared one: JRR_ERR_ARG, before anything is launched.  A scratch below jrr_jfit_norm_bytes:
 *                  JRR_ERR_WORKSPACE.  An ns that is not the prepared NS is found on the device: the error word of the state is set
 *                  (the next jrr_jfit_info reports it) and the output is filled with NaN.                                         */
enum { JRR_JFIT_NORM_UNIT = 0, JRR_JFIT_NORM_INV = 1 };
size_t jrr_jfit_norm_bytes(const int32_t counts[17], size_t* scratch_bytes);
int jrr_jfit_norm_moments(void* state_dev, const void* cache_dev, int64_t n_rows, int64_t begin, int64_t count, int ns,
                          const double* x_dev /* [17][128] */, int mode, double delta_m, double* out_dev, void* scratch_dev,
                          size_t scratch_bytes, void* stream);

/* ---- the price of every mesh vertex in the regressor solve (`--fit_solve --fit_grow R`, regressor_solve.py, csrc/jprice.hip) ------------
 * The solve above is exact over the entries it was given; its Frank-Wolfe gap says nothing about the other vertices of a row.  What is
 * missing is the gradient of the loss with respect to a weight on EVERY vertex at the current solution.  With the residuals of section
 * 3k / 3l (r_i = q_i - q_0 - gt_i / 1000, q_i = sum_e x_i[e] v[vtx_i[e]], rho = sqrt(r.r + delta^2); an empty row is left out, an empty
 * pelvis row means q_0 = 0) and the adjoint  a_i = r_i (JRR_JFIT_PRICE_MSE)  or  a_i = r_i / rho (JRR_JFIT_PRICE_NORM), the pass gives
 *     S[i][u] = sum_s sum_c a_i,c(s) v[s][u][c]          i = 1 .. 16, u = 0 .. 6889                       (fp64 throughout)
 * and the host forms  g_i[u] = 2 S[i][u] / (51 n)  (MSE)  or  S[i][u] / (17 n)  (NORM),  g_0 = - sum_i g_i: at listed vertices exactly the
 * gradient of the solve, elsewhere the reduced cost g_i[u] - lambda_i that certifies the solution over the whole mesh or names the
 * vertices to add (regressor_solve.global_gap, grow_select).  No engine, no body model, no jfit state.
 *
 * jrr_jfit_price_bytes  the bytes of the output (fixed: JRR_JFIT_PRICE_DOUBLES doubles); *scratch_bytes (nullable) receives the bytes of
 *                  the caller-owned scratch for this batch.  batch < 1: both 0.
 * jrr_jfit_price   verts_dev (batch,6890,3) fp32 m, gt_mm_dev (batch,17,3) fp32 pelvis-centred mm.  The lists are HOST arrays:
 *                  vtx_host[17][128] the vertices of each row's entries, counts_host[17], x_host[17][128] the weights (entries behind a
 *                  row's count are not used).  They are validated on the host, so that every refusal happens before a launch, and copied
 *                  into the head of the scratch on the stream; the call waits for that copy (it synchronises the stream once, as
 *                  jrr_jfit_norm_moments does), so the arrays are the caller's again when it returns.  out_dev: S row-major, row i - 1 for joint i (16 * 6890 doubles), then per joint
 *                  i = 1 .. 16 four doubles: sum r.r, sum rho, sum |r|, samples counted.  An empty row gives zeros everywhere.
 *                  accumulate = 0: out is this batch's sums (whatever it held).  accumulate = 1: every element of out gets this batch's
 *                  complete sum added once, so the result is a function of the sequence of batch sizes alone.
 *                  Three launches: the residuals into the scratch, the products (v_mfma_f64_16x16x4_f64: the 16 joints are the M side,
 *                  a tile is 16 vertices, k = 4 samples of one axis) over (tile blocks x sample chunks) into slabs of at most 32 MiB,
 *                  and a finish that adds the slabs in chunk order.  No floating-point atomics: two identical call sequences give the
 *                  same bits.
 *                  JRR_ERR_ARG, with a message and before anything is enqueued: a NULL pointer, misalignment (verts / gt 4 bytes, out /
 *                  scratch 8), batch < 1, a count outside 0 .. 128, a listed vertex outside 0 .. 6889 or repeated in its row, no row
 *                  with entries, an unknown mode, a delta_m that is negative or not finite, or not positive in NORM mode.
 *                  JRR_ERR_WORKSPACE: a scratch below jrr_jfit_price_bytes.                                                       */
enum { JRR_JFIT_PRICE_MSE = 0, JRR_JFIT_PRICE_NORM = 1, JRR_JFIT_PRICE_DOUBLES = 16 * 6890 + 16 * 4 };
size_t jrr_jfit_price_bytes(int batch, size_t* scratch_bytes);
int jrr_jfit_price(const float* verts_dev /* (batch,6890,3) */, const float* gt_mm_dev /* (batch,17,3), pelvis-centred mm */, int batch,
                   const int32_t* vtx_host /* [17][128] */, const int32_t* counts_host /* [17] */, const double* x_host /* [17][128] */,
                   int mode, double delta_m, int accumulate, double* out_dev, void* scratch_dev, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* JRR_H */
