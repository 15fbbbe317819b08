/*
 * niidmix.h — C-ABI of the MI355X (gfx950) neighbour parameter-mixing library (libniidmix.so).
 *
 * The reference hot path is D-SGD's per-round Jacobi mixing
 *     theta'_i = sum_{j in {i} u E(i)} W[j, i] * theta_j
 * implemented in Python/ATen by
 *     d_sgd.average           /root/reference/tools/simulate/algorithm/d_sgd.py:96-116
 *     setup.model.average     /root/reference/tools/setup/model/__init__.py:15-25
 *     d_sgd.update_models     /root/reference/tools/simulate/algorithm/d_sgd.py:29-35
 * over the topology produced by setup.topology.load
 *     /root/reference/tools/setup/topology/__init__.py:4-12 (edges {int: list}, weights fp32 [N,N]).
 *
 * The reference has no FFI of its own (it is pure Python); the binding a maintainer adds is a ctypes
 * stub.  Every entry point below:
 *   - takes plain device pointers and sizes (no torch types), caller-owned buffers;
 *   - is stream-ordered on the given hipStream_t (passed as void*; NULL = default stream), never
 *     synchronises the host, never allocates;
 *   - returns NIIDMIX_OK or an error code; niidmix_last_error() gives a thread-local message.
 * Slabs are row-major fp32 [rows, p] with leading dimension ld (elements).  One row = the flattened
 * parameters of one simulated node in model.parameters() order.
 * Jacobi semantics: every output row is computed from the pre-round input, so x and y must not
 * overlap.  Every entry point that reads one slab and writes another gets the row count and checks
 * the full extents of both (NIIDMIX_EALIAS), each slab with its own strides.
 *
 * ABI 6 (this header): niidmix_sgd_momentum_step_rows_f32 added (the optimizer step of
 * --learning-momentum on the device); niidmix_linear_nll_grad_rows_f32 and its
 * niidmix_linear_nll_grad_rows_scratch_elems added (local training of a linear classifier on the
 * device: forward, loss and backward; a pure addition, the version is unchanged);
 * niidmix_grad_segment_mean_sgd_step_f32 added (the clique gradient mean fused with the optimizer
 * step, for --clique-gradient under --device-training; a pure addition too);
 * niidmix_sample_step_mean_update_f32 added (the 'sample' topology's step, average and broadcast
 * in one launch, for --device-training-sample; a pure addition too); niidmix_draw_batches_i32 and
 * its niidmix_draw_batches_max_len added (training batches drawn on the device, for
 * --device-sampling; a pure addition too); niidmix_epoch_perm_i32, niidmix_take_batches_i32,
 * niidmix_epoch_perm_max_len and niidmix_epoch_perm_scratch_bytes added (a whole epoch's
 * permutation sorted once and sliced every round, for --device-sampling-cached; pure additions too);
 * niidmix_linear_nll_grad_rows_sliced_f32, niidmix_linear_nll_grad_rows_sliced_scratch_elems and
 * niidmix_linear_nll_grad_rows_sliced_slice added (the linear gradient at any batch size, for
 * --device-training-large-batch; pure additions too); niidmix_torch_randperm_i32 and its
 * niidmix_torch_randperm_max_len added (torch.randperm's CPU stream on the device, for
 * --device-sampling-torch-stream; pure additions too).
 * ABI 5: niidmix_dense_split_elems / niidmix_dense_split_w /
 * niidmix_mix_dense_bf16x6_f32 added (the dense GEMM on the bf16 matrix cores, fp32-accurate by
 * three-term splitting); niidmix_mix_strip_f32 refuses a strip that does not fit the device's LDS.
 * ABI 4: niidmix_mix_band_f32 added (banded low-degree graphs, e.g. a ring in its
 * cycle order), niidmix_mix_strip_f32 (column strips for few nodes), register rows in the LDS
 * tile plan.
 * ABI 3: n_rows added to niidmix_mix_tile_f32, niidmix_mix_tile_lds_f32,
 * niidmix_grad_segment_mean_f32 and niidmix_grad_segment_mean_blocked_f32 (full extent checks);
 * niidmix_update_rows_f32 added (the 'sample' topology's broadcast); niidmix_mix_ell_f32 added
 * (low-degree graphs); niidmix_sharded_* / niidmix_mix_sharded_f32 added (sharded round over
 * several GPUs of one process, RCCL); cliques of <= 112 members
 * accept 64-column blocks (the multi-clique tile).
 */
#ifndef NIIDMIX_H
#define NIIDMIX_H

#include <stdint.h>
#include <sys/types.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NIIDMIX_ABI_VERSION 6

enum niidmix_status {
    NIIDMIX_OK = 0,
    NIIDMIX_EINVAL = 1,       /* bad size / pointer / mode argument */
    NIIDMIX_EALIAS = 2,       /* input and output slabs overlap (Jacobi semantics violated) */
    NIIDMIX_EHIP = 3,         /* a HIP runtime call failed (launch error) */
    NIIDMIX_EUNSUPPORTED = 4  /* the plan exceeds what the kernel supports (e.g. clique too large) */
};

enum niidmix_mode {
    /* Bit-exact with the reference loop: for each row, z = x_self*0, acc = z, then in CSR order
     * acc = fl(acc + fl(w*x_j)) (no FMA), finally y = fl(z + acc).  This is setup.model.average's
     * deepcopy/mul_(0)/add_(w*p) (model/__init__.py:19-24) followed by update_models'
     * p.mul_(0.); p.add_(new) (d_sgd.py:31-34). */
    NIIDMIX_MODE_EXACT = 0,
    /* Same terms, fused multiply-add, any association: within the north-star's 1e-5 relative
     * (condition-aware) tolerance, not bitwise. */
    NIIDMIX_MODE_FAST = 1
};

/* OR-ed into `mode`: write the averaged model itself (setup.model.average's return value,
 * model/__init__.py:25) instead of the update_models epilogue fl(x_self*0 + avg).  The two differ
 * only in the sign of an exactly-zero result. */
#define NIIDMIX_FLAG_AVERAGE_ONLY 2

/* OR-ed into `mode` of niidmix_mix_csr_f32: performance hint, the graph's average row length
 * (in-degree + 1) is <= 4 (ring, grid): fewer speculative gathers per batch.  Results unchanged. */
#define NIIDMIX_FLAG_LOW_DEGREE 4

/* OR-ed into `mode` of niidmix_mix_csr_f32: gradient mean instead of parameter mixing.  Row r's
 * entries list the nodes whose gradients it averages (val must be 1.0f), in the reference's order:
 *   acc = +0; acc = fl(acc + g_j) for each entry;  y_r = fl(+0 + fl(acc / row length))
 * = average_gradients (d_sgd.py:19-27: zeros_like, add_, div_(len(models))) followed by
 * update_gradients (d_sgd.py:37-45: grad.zero_(); grad.add_(g)).  Used by --clique-gradient (the
 * clique's members, clique order; with removed clique edges only the members adjacent to the node,
 * d_sgd.py:56-78) and --unbiased-gradient (topology['neighbourhoods'][rank] order, d_sgd.py:79-90).
 * Identical results in EXACT and FAST mode (w = 1: fma(1, g, acc) == fl(acc + g)).  Exclusive with
 * NIIDMIX_FLAG_AVERAGE_ONLY. */
#define NIIDMIX_FLAG_MEAN 8

/* ABI version (NIIDMIX_ABI_VERSION). */
int niidmix_abi_version(void);

/* Thread-local description of the last error returned on this thread ("" if none). */
const char *niidmix_last_error(void);

/* Sparse mixing over a CSR of W^T rows, in the reference's accumulation order.
 * Replaces d_sgd.average (d_sgd.py:96-116) + setup.model.average (model/__init__.py:15-25)
 * + update_models (d_sgd.py:29-35) for all nodes of one round.
 *   x        [>= max(col)+1, ld_x] input slab (device)
 *   y        [n_rows, ld_y] output slab (device), must not overlap x
 *   row_ptr  [n_rows+1] int64 (device); row r's entries are [row_ptr[r], row_ptr[r+1])
 *   col      [nnz] int32 input-row indices (device); the FIRST entry of each row is the node itself
 *            (the reference's models[0] = self, d_sgd.py:105)
 *   val      [nnz] fp32 weights (device): val = W[src, rank] (d_sgd.py:106), self weight first
 *   mode     NIIDMIX_MODE_EXACT or NIIDMIX_MODE_FAST, optionally | NIIDMIX_FLAG_AVERAGE_ONLY
 *            | NIIDMIX_FLAG_LOW_DEGREE | NIIDMIX_FLAG_MEAN
 * Rows with no entries are written as +0. */
int niidmix_mix_csr_f32(const float *x, int64_t ld_x, float *y, int64_t ld_y, int64_t n_rows,
                        int64_t p, const int64_t *row_ptr, const int32_t *col, const float *val,
                        int mode, void *stream);

/* The same round over an ELL layout of the same W^T rows, for low-degree graphs (ring, grid,
 * random regular): row r's entries are ell_col / ell_val[r*k .. r*k + ell_len[r]) in the CSR's
 * order (self first), padded to k entries (the padding is never read as a term).  k: 3, 5 or 8.
 *   x  [>= max(n_rows, max(col)+1), ld_x]: row r's own data (its first entry, normally r itself) is
 *      loaded before its descriptors arrive, so x must hold at least n_rows rows
 * The descriptors are scalar loads (one row per wave) and a wave streams several column chunks of
 * its row.  mode as niidmix_mix_csr_f32 (EXACT / FAST, | NIIDMIX_FLAG_AVERAGE_ONLY); bit-identical
 * to it in EXACT mode. */
int niidmix_mix_ell_f32(const float *x, int64_t ld_x, float *y, int64_t ld_y, int64_t n_rows,
                        int64_t p, int k, const int32_t *ell_col, const float *ell_val,
                        const int32_t *ell_len, int mode, void *stream);

/* The same round for BANDED rows: every entry of row r reads row r + d (mod n_rows) with
 * |d| <= band (a ring in its cycle order: band 1; niidmix.ops.band_layout finds that order and
 * MixCSR.relabel puts the slab in it).  The descriptors are the ELL arrays of niidmix_mix_ell_f32
 * (absolute columns, self first, padded to k); the caller guarantees the band (the kernel folds
 * (col - r) mod n_rows into [-band, band]; an entry outside the band reads a wrong row).  A wave
 * loads its output rows and the band rows around them before any descriptor arrives, so a round is
 * one memory round trip per wave and each row is loaded about once instead of k times.
 * (k, band): (3, 1) or (5, 2); n_rows >= 2 band + 1; p and both ld even, 8-B aligned slabs
 * (NIIDMIX_EUNSUPPORTED otherwise: use niidmix_mix_ell_f32).  x and y: [n_rows, ld].  mode as
 * niidmix_mix_ell_f32; bit-identical to it (and to niidmix_mix_csr_f32) in EXACT mode. */
int niidmix_mix_band_f32(const float *x, int64_t ld_x, float *y, int64_t ld_y, int64_t n_rows,
                         int64_t p, int k, int band, const int32_t *ell_col, const float *ell_val,
                         const int32_t *ell_len, int mode, void *stream);

/* The same round (d_sgd.average, tools/simulate/algorithm/d_sgd.py:96-116) for FEW nodes
 * (n_rows <= 256; ring 100, BASELINE configs[1], tools/setup/topology/ring.py:12-27) by column
 * strips: a block of 8 waves owns a strip of every row -- 256 columns (float4 lanes) when x and y
 * are 16-B aligned, both ld are multiples of 4, ld_x >= p rounded up to 4 and n_rows <= 156, else
 * 64 columns -- stages it in LDS by LDS-DMA and combines each output row from there in its ELL
 * order, so each element of x is read from memory once.  Any row order.  Descriptors: the ELL arrays of
 * niidmix_mix_ell_f32 (k = 3, 5 or 8).  Contract: every ell_col entry is < n_rows -- only rows
 * 0..n_rows-1 are staged, so x must hold exactly the rows the outputs read (a node shard whose
 * rows read halo rows past its own is NOT a strip round: use niidmix_mix_ell_f32); the descriptors
 * are device arrays and are not checked here (niidmix.ops.Mixer checks them once per topology).
 * NIIDMIX_EUNSUPPORTED when the strip does not fit the device's per-block LDS.
 * x 4-B aligned; x and y: [n_rows, ld].  mode as
 * niidmix_mix_ell_f32; bit-identical to it (and to niidmix_mix_csr_f32) in EXACT mode.  Round 4
 * (ABI 4). */
int niidmix_mix_strip_f32(const float *x, int64_t ld_x, float *y, int64_t ld_y, int64_t n_rows,
                          int64_t p, int k, const int32_t *ell_col, const float *ell_val,
                          const int32_t *ell_len, int mode, void *stream);

/* Clique-factored mixing (fast mode only).  For each member m of clique c:
 *   y_m = a_m * x_m + sum_{g < n_groups} c_{m,g} * S_{c,g} + sum_r res_val[r] * x[res_col[r]]
 * with S_{c,g} = sum of x over the members of clique c in group g.  The host derives the plan from
 * the loaded W (topology.json 'cliques', d_cliques/random_cliques.py:18-37 + weights.py:15-25) and
 * verifies that it reproduces every W entry; see DESIGN.md.  All arrays are device pointers.
 *   clique_ptr   [n_cliques+1] int32 offsets into the member arrays
 *   member_row   [n_members] int32 row index (input row == output row)
 *   member_group [n_members] int32 group id in [0, n_groups), optionally OR-ed with
 *                NIIDMIX_MEMBER_GATEWAY when the member's row is also some residual entry's source
 *                (res_col): a load-policy hint only (that row is loaded temporally so the gather
 *                hits L2), never changes results
 *   coef         [n_members * (1 + n_groups)] fp32: a_m, then c_{m,0..n_groups-1}
 *   res_ptr      [n_members+1] int32 offsets into res_col/res_val (residual sparse terms)
 *   res_col      [n_res] int32 input rows, res_val [n_res] fp32
 *   res_member   [n_res] int32 index, within its clique, of the member each residual entry belongs
 *                to (the register tile fetches a clique's residual entries lane-parallel together
 *                with the member descriptors, so the gateway-row gathers issue right behind the
 *                member-row loads)
 *   max_clique   largest clique size: <= 256 selects a register tile (one HBM read per
 *                parameter); 257..1024 (e.g. fully-connected = one clique) the one-pass
 *                big-clique kernel (a 32-column item of every member held in registers, one HBM
 *                read per parameter); larger cliques a two-pass kernel (rows read twice)
 *   max_clique_res  largest number of residual terms of one clique (informational, >= 0)
 *   n_groups     1..4
 *   csr_ptr / csr_col / csr_val   the CSR of the same W^T (niidmix_mix_csr_f32's row_ptr / col /
 *                val, rows indexed like member_row): the non-finite guard.  The factored form
 *                combines every member into every output, the reference only a node's real edges
 *                (d_sgd.py:105-106) on top of self*0 (model/__init__.py:20-21); every output the
 *                kernel finds non-finite is recomputed from its CSR row (fast-mode arithmetic), so
 *                inf / NaN propagate exactly along real edges and a non-finite self gives NaN.
 * Range checks: x and y must not overlap over the member rows (NIIDMIX_EALIAS). */
#define NIIDMIX_MEMBER_GATEWAY 256

typedef struct niidmix_clique_plan {
    int32_t n_cliques;
    int32_t n_members;
    int32_t n_groups;
    int32_t max_clique;
    int32_t max_clique_res;
    const int32_t *clique_ptr;
    const int32_t *member_row;
    const int32_t *member_group;
    const float *coef;
    const int32_t *res_ptr;
    const int32_t *res_col;
    const float *res_val;
    const int32_t *res_member;
    const int64_t *csr_ptr;
    const int32_t *csr_col;
    const float *csr_val;
} niidmix_clique_plan;

int niidmix_mix_clique_f32(const float *x, int64_t ld_x, float *y, int64_t ld_y, int64_t p,
                           const niidmix_clique_plan *plan, void *stream);

/* The same clique-factored round on COLUMN-BLOCKED slabs: x and y are [K][rows][block_cols]
 * (K = ceil(p / block_cols) blocks of row-major [rows, block_cols] sub-slabs with row stride `ld`
 * floats and block strides block_stride_x / block_stride_y floats), element (r, c) at
 *   base + (c / block_cols) * block_stride + r * ld + c % block_cols.
 * block_cols: a power of two >= 256 (the register tile's 256-column chunks), >= 64 when
 * max_clique <= 112 (the multi-clique tile's 64-column items, which also serves every plan with
 * >= 4096 member rows: Q = 4 cliques per item keep a column chunk's rows in an XCD's L2), >= 32
 * when max_clique > 256 (the big-clique kernel's 32-column items).  This is the layout niidmix keeps
 * device-resident node state in (Mixer.device_layout: block_cols = 1024 for cliques of <= 256
 * members, 256 when a clique has > 64 gateway terms, 32 for big cliques; clique-contiguous rows),
 * which measured robust to the slab's physical placement.  Cliques of <= 256 members use
 * the register tile, 257..1024 members the one-pass big-clique kernel (32-column items). */
int niidmix_mix_clique_blocked_f32(const float *x, float *y, int64_t p, int64_t ld,
                                   int64_t block_cols, int64_t block_stride_x,
                                   int64_t block_stride_y, const niidmix_clique_plan *plan,
                                   void *stream);

/* Merged-order row tiles, exact or fast: the same result as niidmix_mix_csr_f32 (bit for bit in
 * NIIDMIX_MODE_EXACT: every row keeps its own operand order — self, then edges[rank] in list order,
 * d_sgd.py:105-106 — and its own roundings), computed so that rows sharing sources share the loads.
 * Output rows are cut into tiles of rt rows (e.g. parts of a clique).  Each tile has one merged list
 * of positions such that every row's entry list (self excluded) is a subsequence of it; a position
 * names a source row, the tile rows that take it (mask) and their weights.  Built on the host by
 * niidmix.tile.build_tile_plan.
 *   n_sub      tiles;  rt  rows per tile: 8, 16 or 32
 *   sub_ptr    [n_sub+1] int64 offsets into the position arrays
 *   sub_rows   [n_sub*rt] int32 output rows, -1 for an unused slot
 *   sub_wself  [n_sub*rt] fp32 W[r, r] of each tile row (its first CSR entry)
 *   pos_src    [L] int32 source row of every position, | NIIDMIX_TILE_POS_UNIFORM when every
 *              slot of the position's pos_w holds the same fp32 value (exact mode then forms the
 *              product fl(w*x) once per position and adds it to each taking row: same bits)
 *   pos_mask   [L] uint32: bit r set when tile row r takes the position (unused slots: set)
 *   pos_w      [L*rt] fp32 weight W[src, row] per tile row (0 where the row skips the position)
 *   (pos_* must be valid device pointers even when L == 0; they are read only inside sub_ptr ranges)
 * mode: NIIDMIX_MODE_EXACT / _FAST, optionally | NIIDMIX_FLAG_AVERAGE_ONLY. */
#define NIIDMIX_TILE_POS_UNIFORM (1 << 30)
typedef struct niidmix_tile_plan {
    int64_t n_sub;
    int32_t rt;
    int32_t reserved;
    const int64_t *sub_ptr;
    const int32_t *sub_rows;
    const float *sub_wself;
    const int32_t *pos_src;
    const uint32_t *pos_mask;
    const float *pos_w;
} niidmix_tile_plan;

int niidmix_mix_tile_f32(const float *x, int64_t ld_x, float *y, int64_t ld_y, int64_t n_rows,
                         int64_t p, const niidmix_tile_plan *plan, int mode, void *stream);

/* LDS-staged merged-order row tiles (exact-mode default for clique topologies): the same tiles and
 * results as niidmix_mix_tile_f32 (bit for bit in NIIDMIX_MODE_EXACT), grouped: a group (a clique)
 * owns consecutive tiles and a list of the DISTINCT source rows its tiles read.  One workgroup per
 * (group, 128-column chunk) stages those rows' columns in LDS (one HBM read per row), then each
 * wave applies one tile's positions from LDS.  Built by niidmix.tile.build_tile_lds_plan.
 *   rt, n_sub, sub_ptr, sub_rows, sub_wself, pos_mask, pos_w   as niidmix_tile_plan
 *   pos_slot     [L] int32 index of the position's source in its group's grp_src_rows list
 *                (| NIIDMIX_TILE_POS_UNIFORM as for niidmix_tile_plan.pos_src)
 *   sub_slot     [n_sub*rt] int32 index of each tile row's own row in the group list (0 for unused)
 *   n_grp        groups;  grp_tile_ptr [n_grp+1] int32 tile ranges;  max_tiles = most tiles in a
 *                group: 1..16 for rt 8, 1..12 for rt 16, 1..4 for rt 32 (64*max_tiles threads)
 *   grp_src_ptr  [n_grp+1] int32;  grp_src_rows  int32 source rows;  max_src = largest list (<= 256:
 *                max_src * 512 B of LDS)
 * Needs even p and ld and 8-B aligned slabs (2 columns per lane).  mode as niidmix_mix_tile_f32. */
typedef struct niidmix_tile_lds_plan {
    int64_t n_sub;
    int32_t rt, n_grp, max_src, max_tiles;
    const int64_t *sub_ptr;
    const int32_t *sub_rows;
    const int32_t *sub_slot;
    const float *sub_wself;
    const int32_t *pos_slot;
    const uint32_t *pos_mask;
    const float *pos_w;
    const int32_t *grp_tile_ptr;
    const int32_t *grp_src_ptr;
    const int32_t *grp_src_rows;
    /* optional (rt 16; NULL = the per-position loop): the positions cut into segments, runs read
     * from consecutive LDS slots with immediate offsets (niidmix.tile.build_tile_segments):
     *   seg_ptr [n_sub+1] int32 segments of each tile;  seg [n_seg * 4] int32 per segment:
     *   a run: first slot | length << 12 | first skipped tile row << 20, weight-select bits, skip
     *   bits, 0;  a masked position: slot | 1 << 30, the tile rows that take it, its weight (fp32
     *   bits), 0;  seg_w [n_sub * 2] fp32 the tile's two weights */
    const int32_t *seg_ptr;
    const int32_t *seg;
    const float *seg_w;
    /* optional (rt 16 with segments, EXACT mode; NULL = the segment walker): the positions as
     * matrix-core lists (niidmix.tile.build_tile_mfma_positions), applied by v_mfma_f32_16x16x4_f32
     * 4 positions at a time, bit-identical; a block whose staged rows hold a non-finite value or
     * one below 1e-30 in magnitude takes the segment walker instead:
     *   mf_ptr [n_sub+1] int32 entries of each tile (multiples of 4);  mf [n_mf * 4] int32 per
     *   entry: slot, weight (fp32 bits), tile rows that take it, 0 */
    const int32_t *mf_ptr;
    const int32_t *mf;
    /* optional (rt 16 with segments, mf_ptr NULL; NULL = every source staged in LDS): REGISTER
     * rows, sources outside a group that only masked entries read (a gateway row's inter-clique
     * neighbour), kept per tile in registers instead of the LDS stage
     * (niidmix.tile.build_tile_lds_plan(remote_regs=True)):  rem_rows [n_sub * 16] int32 global
     * rows of each tile's register rows (-1 unused); a masked segment whose word 0 has bit 29 set
     * reads register row (word 0 & 0xfff).  Round 4 (ABI 4). */
    const int32_t *rem_rows;
    /* register rows the kernel loads per tile: 8 (every tile's rem_rows entries 8..15 are -1; 16
     * fewer VGPRs, so three 7-wave blocks fit a CU) or 16; 0 = 16; -16: all 16 in two phases of 8
     * in the 8-row kernel's registers, 8..15 loaded when the walk reaches the first segment that
     * reads one -- only for plans whose tiles read rows 0..7 before any of 8..15
     * (niidmix.tile.rem_two_phase) */
    int32_t rem_regs;
} niidmix_tile_lds_plan;

int niidmix_mix_tile_lds_f32(const float *x, int64_t ld_x, float *y, int64_t ld_y, int64_t n_rows,
                             int64_t p, const niidmix_tile_lds_plan *plan, int mode, void *stream);

/* Dense mixing Y = W^T X on the fp32 matrix cores (v_mfma_f32_32x32x2_f32), for topologies dense
 * enough that W x Theta is a genuine GEMM (fully-connected, tools/setup/topology/fully-connected.py).
 *   w  [n, n] fp32 row-major, w[src*n + dst] = W[src, dst] — the reference's topology['weights']
 *      layout (topology/__init__.py:9) — device pointer
 *   x  [n, ld_x], y [n, ld_y]
 *   row_ptr / col / val   the CSR of the same W^T (as niidmix_mix_csr_f32): the non-finite guard
 *      (see niidmix_clique_plan.csr_ptr) — an output the GEMM finds non-finite (W = 0 off the edges
 *      gives 0*inf = NaN) is recomputed from its node's real edges. */
int niidmix_mix_dense_f32(const float *x, int64_t ld_x, float *y, int64_t ld_y, int64_t n,
                          int64_t p, const float *w, const int64_t *row_ptr, const int32_t *col,
                          const float *val, void *stream);

/* The same GEMM on the BF16 matrix cores with fp32 accuracy (round 5, ABI 5): each fp32 operand is
 * split into three bf16 terms (a = a_h + a_m + a_l, residue < 2^-24 |a|) and the six partial
 * products reaching 2^-16 |a b| are accumulated in fp32 by v_mfma_f32_32x32x16_bf16 -- on gfx950 the
 * fp32-input MFMA runs at 1/16 of the bf16 rate, so six bf16 products cost 6/16 of one fp32 one.
 * The error is of the order of one fp32 rounding per product (fast mode's 1e-5 condition-aware
 * tolerance, like the fp32 kernel); non-finite outputs are recomputed from the CSR as above.
 *   wp  the split W^T from niidmix_dense_split_w (device, 16-B aligned,
 *       niidmix_dense_split_elems(n) uint16 elements); made once per topology.
 * Other arguments as niidmix_mix_dense_f32. */
int64_t niidmix_dense_split_elems(int64_t n);
int niidmix_dense_split_w(const float *w, int64_t n, uint16_t *wp, void *stream);
int niidmix_mix_dense_bf16x6_f32(const float *x, int64_t ld_x, float *y, int64_t ld_y, int64_t n,
                                 int64_t p, const uint16_t *wp, const int64_t *row_ptr,
                                 const int32_t *col, const float *val, void *stream);

/* Column mean over rows (the uniform global average of setup.model.average(models) with
 * weights=None, model/__init__.py:17-18, used by d_sgd.init :137-141 and the logger :112,260),
 * with the per-row squared L2 distance to that mean (logger.model_distance, logger.py:42-48).
 *   mean  [p] fp32 output;  dist2 [n] fp64 output (may be NULL)
 *   mode EXACT reproduces the reference's left-to-right fl(acc + fl(w*x_k)) with w = fp32(1/n). */
int niidmix_mean_rows_f32(const float *x, int64_t ld_x, int64_t n, int64_t p, float *mean,
                          double *dist2, int mode, void *stream);

/* Segment gradient mean for --clique-gradient without removed clique edges (d_sgd.py:56-65):
 * segment s lists the member rows seg_row[seg_ptr[s] .. seg_ptr[s+1]) in clique order, and EVERY
 * member row of y receives the same mean of the members' rows of g:
 *   acc = +0; acc = fl(acc + g_m) in member order; y_m = fl(+0 + fl(acc / len))
 * = average_gradients (d_sgd.py:19-27) + update_gradients (d_sgd.py:37-45), bit for bit.  One read
 * of every member row and one write (HBM-bound), instead of len gathers per output row.
 *   g  [n_rows, ld_g] gradient slab (device), y [n_rows, ld_y] output (device, must not overlap g)
 *   seg_ptr [n_seg+1], seg_row [seg_ptr[n_seg]] int32 (device).  Rows in no segment are untouched. */
int niidmix_grad_segment_mean_f32(const float *g, int64_t ld_g, float *y, int64_t ld_y,
                                  int64_t n_rows, int64_t p, int64_t n_seg, const int32_t *seg_ptr,
                                  const int32_t *seg_row, void *stream);

/* niidmix_grad_segment_mean_f32 on column-blocked slabs [K][rows][block_cols] (see
 * niidmix_mix_clique_blocked_f32; block_cols a power of two >= 1024, p % 4 == 0). */
int niidmix_grad_segment_mean_blocked_f32(const float *g, float *y, int64_t n_rows, int64_t p,
                                          int64_t ld, int64_t block_cols, int64_t block_stride_g,
                                          int64_t block_stride_y, int64_t n_seg,
                                          const int32_t *seg_ptr, const int32_t *seg_row,
                                          void *stream);

/* SGD step on the listed rows: p[row] = fma(neg_lr, g[row], p[row]) — torch.optim.SGD with
 * momentum 0 and no weight decay (param.add_(grad, alpha=-lr); ATen's CPU kernel fuses it into one
 * fma with an fp32 alpha), the optimizer step the reference runs after gradient averaging
 * (d_sgd.py:63-64, :77-78, :88-90).  The fused drop-in round (niidmix.d_sgd) runs gradient mean ->
 * this step -> mixing on each device window, so the step never visits the host.
 *   p [*, ld_p] parameters (device, updated in place), g [*, ld_g] gradients (device)
 *   rows [n_rows] int32 rows to step (device) */
int niidmix_sgd_step_rows_f32(float *p, int64_t ld_p, const float *g, int64_t ld_g, int64_t ncols,
                              const int32_t *rows, int64_t n_rows, float neg_lr, void *stream);

/* SGD step with momentum on the listed rows — torch.optim.SGD(lr, momentum) without dampening,
 * weight decay or Nesterov, the optimizer the reference builds from --learning-momentum
 * (d_sgd.py:118-122) and steps at d_sgd.py:52, :65, :80, :92.  Bit for bit ATen's CPU arithmetic:
 *   first != 0 (a parameter's first step):  buf[row] = g[row]   (a copy: -0.0 stays -0.0; buf is
 *                                                                not read)
 *   first == 0:   buf[row] = fl(fl(momentum * buf[row]) + g[row])   (buf.mul_(m).add_(g): the
 *                                                                multiply and the add round apart)
 *   then always:  p[row]   = fma(neg_lr, buf[row], p[row])      (p.add_(buf, alpha=-lr): one rounding)
 * with neg_lr = fp32(-lr) and momentum = fp32(m).  One streaming pass: p, g and buf are read and p
 * and buf written (20 B per element; 16 B with `first`).  Rows not listed are untouched in p and buf.
 * The resident drop-in round (niidmix.d_sgd) runs gradient mean -> this step -> mixing with buf
 * kept in HBM between rounds.
 *   p   [*, ld_p] parameters (device, updated in place)
 *   g   [*, ld_g] gradients (device)
 *   buf [*, ld_b] momentum buffers (device, updated in place)
 *   rows [n_rows] int32 distinct rows to step (device)
 * Range checks: the row list is on the device and is not read by the launcher, so each slab's
 * extent is taken as the least n_rows distinct rows can span, (n_rows - 1) * ld + ncols elements
 * from its base; any two of p, g, buf that overlap over those extents are refused (NIIDMIX_EALIAS).
 * NIIDMIX_EINVAL: a null pointer, a negative size, a leading dimension below ncols. */
int niidmix_sgd_momentum_step_rows_f32(float *p, int64_t ld_p, const float *g, int64_t ld_g,
                                       float *buf, int64_t ld_b, int64_t ncols,
                                       const int32_t *rows, int64_t n_rows, float neg_lr,
                                       float momentum, int first, void *stream);

/* Segment gradient mean fused with the SGD step: --clique-gradient without removed clique edges on
 * device-resident parameters (niidmix.train.DeviceTrainer), i.e. the reference's average_gradients,
 * update_gradients and optimizer.step() of every clique member (d_sgd.py:56-65) in one pass.
 * Segment s lists the member rows seg_row[seg_ptr[s] .. seg_ptr[s+1]) in clique order; segments are
 * disjoint.  Per segment and column:
 *   acc = +0; acc = fl(acc + g_m) in member order; gm = fl(+0 + fl(acc / len))
 *   momentum == 0:  p_m = fma(neg_lr, gm, p_m)                  (buf may be NULL, first is ignored)
 *   first != 0:     buf_m = gm (a copy; buf is not read);         p_m = fma(neg_lr, buf_m, p_m)
 *   otherwise:      buf_m = fl(fl(momentum * buf_m) + gm);       p_m = fma(neg_lr, buf_m, p_m)
 * for every member m: bit for bit niidmix_grad_segment_mean_f32 followed by
 * niidmix_sgd_step_rows_f32 / niidmix_sgd_momentum_step_rows_f32 over the member rows, without the
 * averaged gradient slab: g, p (and buf) are read and p (and buf) written once, 12 B per
 * node-parameter without momentum, 16 B on the first momentum step and 20 B later, against 20 / 24
 * / 28 B for the two calls.  g is not written.  Rows in no segment and columns from ncols to the
 * leading dimension are untouched in p and buf; n_seg == 0 and empty segments are no-ops.
 *   p   [*, ld_p] parameters (device, updated in place)
 *   g   [*, ld_g] gradients (device)
 *   buf [*, ld_b] momentum buffers (device, updated in place); NULL, 0 when momentum == 0
 *   seg_ptr [n_seg+1], seg_row [n_members] int32 (device), n_members = seg_ptr[n_seg]
 * float4 accesses when ncols and the leading dimensions are multiples of 4 and the pointers 16-B
 * aligned, scalar ones otherwise.
 * Range checks: the segment lists are on the device and are not read by the launcher, so each
 * slab's extent is taken as the least n_members distinct rows can span, (n_members - 1) * ld +
 * ncols elements from its base; any two of p, g, buf that overlap over those extents are refused
 * (NIIDMIX_EALIAS; the rule of niidmix_sgd_momentum_step_rows_f32).  NIIDMIX_EINVAL: a null
 * pointer (buf only when momentum != 0), a negative size, a leading dimension below ncols. */
int niidmix_grad_segment_mean_sgd_step_f32(float *p, int64_t ld_p, const float *g, int64_t ld_g,
                                           float *buf, int64_t ld_b, int64_t ncols, int64_t n_seg,
                                           const int32_t *seg_ptr, const int32_t *seg_row,
                                           int64_t n_members, float neg_lr, float momentum, int first,
                                           void *stream);

/* The 'sample' topology's round on device-resident parameters (niidmix.train.DeviceTrainer under
 * --device-training-sample) in one launch: the optimizer step of the k sampled rows, their average
 * setup.model.average(models, [1/k]*k) in the sample's order, and update_models of EVERY row
 * (d_sgd.py:236-250).  Per column:
 *   for j in 0..k-1, r = active[j]:
 *     b   = g[r]                                if momentum == 0 or first[j] != 0
 *         = fl(fl(momentum * buf[r]) + g[r])    otherwise       (two roundings, no FMA)
 *     if momentum != 0: buf[r] = b                              (a copy keeps -0.0)
 *     t_j = fma(neg_lr, b, x[r])                                (one rounding)
 *   acc = fl(t_0 * 0);  for j in 0..k-1: acc = fl(acc + fl(w * t_j))     (no FMA, in this order)
 *   for every row i: y[i] = fl(fl(s_i * 0) + acc),  s_i = t_j if i == active[j], else x[i]
 * with w = fp32(1/k) (1/k computed in double, then rounded).  Bit for bit
 * niidmix_sgd_step_rows_f32 / niidmix_sgd_momentum_step_rows_f32 over the active rows, then
 * niidmix_mix_csr_f32 (NIIDMIX_MODE_EXACT | NIIDMIX_FLAG_AVERAGE_ONLY, one output row) over them,
 * then niidmix_update_rows_f32, except that x is not written: the stepped parameters exist only
 * inside the launch.  g is not written either; rows of buf that are not listed, and columns from
 * ncols to the leading dimension of y and buf, are untouched.
 *   x      [n_rows, ld_x] parameters before the round (device)
 *   y      [n_rows, ld_y] parameters after it (device), must not overlap x
 *   g      [*, ld_g] gradients (device), buf [*, ld_b] momentum buffers (device; NULL, 0 when
 *          momentum == 0)
 *   active [k] int32 distinct rows in the sample's order (device)
 *   first  [k] int32, non-zero where the row takes its first momentum step (device; NULL when
 *          momentum == 0)
 * How the last line gets s_i of a sampled row: a thread owns its columns and walks the rows
 * itself, so every element of y and buf has exactly one writer and no thread reads what another
 * writes.  fl(s_i * 0) matters only through its sign and finiteness, and those can show only
 * when acc is +-0, inf or NaN: a finite non-zero acc means every t_j (hence every sampled x[r])
 * was finite, and fl(+-0 + acc) = acc for sampled and other rows alike.  So the walk over all
 * rows uses x[i] for every row, and only a thread whose acc is +-0, inf or NaN goes over the
 * sample once more and recomputes t_j from x[r] and b (g[r], or buf[r] as it has just written it).
 * There is neither a row -> slot map nor a stash in y.  Traffic per node-parameter: 4 (2 n_rows +
 * 2k) B without momentum, + 4k B for the buffer written, + 4k B more where it is read, against
 * 4 (2 n_rows + 4k / 5k / 6k) B for the three calls.
 * float4 accesses when ncols and the leading dimensions are multiples of 4 and the pointers 16-B
 * aligned, scalar ones otherwise.
 * Range checks: the lists are on the device and are not read by the launcher.  x and y are taken
 * over all n_rows rows; g and buf over the least k distinct rows can span, (k - 1) * ld + ncols
 * elements.  NIIDMIX_EALIAS: y overlaps x, g or buf, or buf overlaps x or g.  NIIDMIX_EINVAL: a null
 * pointer (buf and first only when momentum != 0), a negative size, k < 1, k > n_rows, a leading
 * dimension below ncols. */
int niidmix_sample_step_mean_update_f32(const float *x, int64_t ld_x, float *y, int64_t ld_y,
                                        const float *g, int64_t ld_g, float *buf, int64_t ld_b,
                                        const int32_t *active, const int32_t *first, float w,
                                        float neg_lr, float momentum, int64_t ncols, int64_t n_rows,
                                        int64_t k, void *stream);

/* Local training of a linear classifier on the listed rows: forward, mean NLL loss and backward of
 * the reference's linear model (setup/model/linear.py: one nn.Linear(K, C), log_softmax, nll_loss)
 * over each row's own batch, i.e. F.nll_loss(F.log_softmax(fc(x.view(-1, K)), 1), y).backward() on
 * a zeroed gradient, for every listed node in one call (the drop-in's --device-training round:
 * this call -> niidmix_sgd_step_rows_f32 / niidmix_sgd_momentum_step_rows_f32 -> mixing, the
 * parameters never leaving HBM).
 *   theta     [*, ld_t] parameters (device); row r is W as [C, K] row-major, then b [C]
 *             (model.parameters() order), P = C * K + C columns
 *   data      [S, K] samples (device), labels [S] int32 classes (device)
 *   batch_idx [n_rows, b_max] int32 sample indices into data (device); entry i belongs to rows[i]
 *   batch_len [n_rows] int32, 1 <= len <= b_max (device): entries past len are not read
 *   rows      [n_rows] int32 distinct slab rows (device)
 *   grad      [*, ld_g] gradients (device), row layout of theta: all P elements of a listed row are
 *             written, other rows and columns past P are untouched
 *   loss      [n_rows] mean batch loss of rows[i] (device)
 *   scratch   caller-owned device buffer of at least
 *             niidmix_linear_nll_grad_rows_scratch_elems(n_rows, b_max, C) floats (partial logits,
 *             then dz); its contents are overwritten
 * With z[s,c] = sum_k x[s,k] W[c,k] + b[c], m_s = max_c z[s,c], lse_s = m_s + log sum_c
 * exp(z[s,c] - m_s):  loss = -(1/len) sum_s (z[s,y_s] - lse_s),  dz[s,c] = (exp(z[s,c] - lse_s) -
 * [c == y_s]) / len,  dW[c,k] = sum_s dz[s,c] x[s,k],  db[c] = sum_s dz[s,c].
 * fp32 FMAs in an order fixed by the launch shape (the sizes, leading dimensions and pointer
 * alignments), no floating-point atomics: two calls on the same inputs give the same bits.  Not
 * bit-identical to ATen's CPU result (another summation order); within 1e-5 of the
 * condition-aware bound sum_s (p[s,c] + [c == y_s]) / len * |x[s,k]| (tests/test_gpu_train.py).
 * Limits (NIIDMIX_EUNSUPPORTED beyond): C <= 1024, b_max * C <= 32768 (one row's dz in LDS),
 * K <= 2^20.  float4 accesses when K and the leading dimension are multiples of 4 and the
 * pointers 16-B aligned, scalar ones otherwise (any K, any ld).
 * NIIDMIX_EINVAL: a null pointer, a negative or zero size, ld_t or ld_g < C * K + C, a scratch
 * buffer that is too small.  NIIDMIX_EALIAS: grad (or scratch) overlaps theta over the least
 * extent n_rows distinct rows can span, (n_rows - 1) * ld + P elements (the row list is on the
 * device and is not read by the launcher, as for niidmix_sgd_momentum_step_rows_f32).
 * batch_idx, batch_len, labels and rows are device data and are NOT checked by the launcher: an
 * index outside data reads out of bounds (batch_len is clamped to [0, b_max]; a label outside
 * [0, C) matches no class).  niidmix.train.DeviceTrainer checks them once per node set. */
int64_t niidmix_linear_nll_grad_rows_scratch_elems(int64_t n_rows, int64_t b_max, int64_t C);
int niidmix_linear_nll_grad_rows_f32(const float *theta, int64_t ld_t, const float *data,
                                     const int32_t *labels, const int32_t *batch_idx,
                                     const int32_t *batch_len, int64_t b_max, const int32_t *rows,
                                     int64_t n_rows, float *grad, int64_t ld_g, float *loss,
                                     int64_t K, int64_t C, float *scratch, int64_t scratch_elems,
                                     void *stream);

/* niidmix_linear_nll_grad_rows_f32 at any batch size (the drop-in's --device-training-large-batch:
 * few nodes with long batches, down to the reference's centralised baseline of one node and
 * batches of 12 800).  The arguments, their order, the loss and gradient computed, the argument
 * checks, the error codes and the clamping of batch_len to [0, b_max] are those of
 * niidmix_linear_nll_grad_rows_f32; only the limits and the scratch differ:
 *   Limits (NIIDMIX_EUNSUPPORTED beyond): C <= 1024, K <= 2^20, 1 <= b_max <= 2^20; a scratch size
 *   beyond int64 or a grid beyond int32.
 *   scratch   at least niidmix_linear_nll_grad_rows_sliced_scratch_elems(n_rows, b_max, K, C)
 *             floats (0 for a non-positive size): the partial logits / dz, one partial gradient
 *             row of P floats (padded to 4) per (row, slice), one loss partial per (row, slice).
 * A batch is cut into slices of S = niidmix_linear_nll_grad_rows_sliced_slice(C) samples, slice q =
 * samples [qS, min((q + 1) S, len)): S is the largest power of two with S * C <= 8192 and
 * S <= 1024 (0 for a C outside 1..1024), a function of C alone, so that a slice's dz takes
 * S * C * 4 <= 32768 bytes of LDS and five workgroups share a CU.  Four launches: the partial
 * logits as in niidmix_linear_nll_grad_rows_f32; per (row, slice) the max-subtracted softmax, dz
 * divided by the WHOLE batch's len and the slice's loss partial; per (row, slice, column chunk,
 * class block) the slice's dW / db into the partial gradients, a lane summing the slice's samples
 * in order; per (row, column) the partials summed in slice order into grad, and loss =
 * -(sum of the loss partials in slice order) / len.  Slices that start at or past len are skipped
 * by every launch.  A row with len = 0 gets a zero gradient and the loss 0 / 0, as from
 * niidmix_linear_nll_grad_rows_f32.
 * No floating-point atomics: every output bit is a function of (n_rows, b_max, K, C), the leading
 * dimensions, the pointer alignments and the inputs alone.  Of the four sizes the SUMMATION ORDER
 * depends on n_rows and K (the K-chunks of the partial logits, as in
 * niidmix_linear_nll_grad_rows_f32) and on C (the slice length S and the lanes per sample of the
 * softmax); it does not depend on b_max, which only sizes the scratch: a batch gives the same bits
 * under any b_max >= len.  Not bit-identical to niidmix_linear_nll_grad_rows_f32 where both take a
 * shape (the slices are another order); both are within 1e-5 of the condition-aware bound
 * (tests/test_gpu_train_large_batch.py). */
int64_t niidmix_linear_nll_grad_rows_sliced_slice(int64_t C);
int64_t niidmix_linear_nll_grad_rows_sliced_scratch_elems(int64_t n_rows, int64_t b_max, int64_t K,
                                                          int64_t C);
int niidmix_linear_nll_grad_rows_sliced_f32(const float *theta, int64_t ld_t, const float *data,
                                            const int32_t *labels, const int32_t *batch_idx,
                                            const int32_t *batch_len, int64_t b_max, const int32_t *rows,
                                            int64_t n_rows, float *grad, int64_t ld_g, float *loss,
                                            int64_t K, int64_t C, float *scratch, int64_t scratch_elems,
                                            void *stream);

/* Evaluation of a linear classifier on the listed rows: what the reference's logger computes per
 * node on the CPU (model.forward + F.nll_loss(reduction='sum') + argmax over a DataLoader), for
 * every job in one call (the drop-in's --device-evaluation; niidmix.evaluate.DeviceEvaluator).
 * Job i evaluates slab row rows[i] on the contiguous samples data[seg_start[i] .. seg_start[i] +
 * seg_len[i]).  rows may repeat and segments may coincide (a shared test set is every job with
 * seg_start = 0); nothing in theta is written.
 *   theta     [*, ld_t] parameters (device), the row layout of niidmix_linear_nll_grad_rows_f32:
 *             W as [C, K] row-major, then b [C]; P = C * K + C columns
 *   data      [S, K] samples (device), labels [S] int32 classes (device)
 *   rows, seg_start, seg_len   [n_jobs] int32 (device); seg_len[i] is clamped to [0, max_len]
 *   loss_sum  [n_jobs] double (device): sum_s nll_s; each nll_s is fp32 and they are added in
 *             double, in sample order within a tile of 64 samples, the tiles in tile order
 *   correct   [n_jobs] int32 (device): #{s : pred_s == y_s}
 *   pred      NULL, or [n_jobs, ld_pred] int32 (device): pred[i * ld_pred + j] is the prediction for
 *             job i's j-th sample; entries at or past seg_len[i] are untouched
 *   scratch   caller-owned device buffer (8-B aligned) of at least
 *             niidmix_linear_eval_rows_scratch_bytes(n_jobs, max_len, C) bytes (per (job, tile)
 *             partial sums and counts); its contents are overwritten
 * With z[s,c] = b[c] + sum_k x[s,k] W[c,k]:  pred_s is the lowest class index that attains the
 * maximum, a NaN logit counting as the maximum and the first NaN winning (torch.argmax /
 * torch.max(.., 1) on the CPU);  nll_s = m_s + log sum_c exp(z[s,c] - m_s) - z[s,y_s], m_s = max_c
 * z[s,c].  A job of length 0 gets 0.0 and 0.
 * fp32 FMAs, every logit one chain over k = 0 .. K-1; no floating-point atomics (the partial
 * results of a (job, tile) go to scratch and a second, small launch adds them in tile order): two
 * calls on the same inputs give the same bits, a job's outputs do not depend on which other jobs
 * the call lists, and an inf or NaN in one row's parameters stays in the jobs that list that row.
 * Not bit-identical to ATen's CPU result (another summation order): loss_sum within 1e-5 of the
 * condition-aware bound sum_s 2 A_s, A_s = max_c (|b_c| + sum_k |x[s,k]| |W[c,k]|), and pred equal to
 * the float64 argmax wherever the top two float64 logits are more than 2e-5 A_s apart
 * (tests/test_gpu_eval.py).
 * Limits (NIIDMIX_EUNSUPPORTED beyond): C <= 1024, K <= 2^20, at most 2^31 - 1 (job group, tile)
 * blocks.  float4 accesses when K and ld_t are multiples of 4 and theta and data 16-B aligned,
 * scalar ones otherwise (any K, any ld_t >= P).
 * Checked before anything touches the GPU, in this order:
 *   NIIDMIX_EINVAL        a null pointer other than pred
 *   NIIDMIX_EINVAL        n_jobs, K or C < 1, max_len < 0
 *   NIIDMIX_EUNSUPPORTED  C > 1024, K > 2^20
 *   NIIDMIX_EINVAL        ld_t < C * K + C
 *   NIIDMIX_EINVAL        ld_pred < max_len (pred given)
 *   NIIDMIX_EINVAL        a scratch buffer that is too small or not 8-B aligned
 *   NIIDMIX_EALIAS        loss_sum, correct, pred or scratch overlaps theta.  The row list is on
 *                         the device, is not read by the launcher and may repeat, so the extent
 *                         taken for theta is the one row every call reads, P elements from its
 *                         base (niidmix::linear_eval_rows checks the whole slab).
 * rows, seg_start, seg_len and labels are device data and are NOT checked by the launcher: a row
 * or a segment outside its array reads out of bounds (a label outside [0, C) matches no class).
 * niidmix.evaluate.DeviceEvaluator checks them once per registered set and builds the job lists
 * itself. */
int64_t niidmix_linear_eval_rows_scratch_bytes(int64_t n_jobs, int64_t max_len, int64_t C);
int niidmix_linear_eval_rows_f32(const float *theta, int64_t ld_t, const float *data,
                                 const int32_t *labels, const int32_t *rows,
                                 const int32_t *seg_start, const int32_t *seg_len, int64_t n_jobs,
                                 int64_t max_len, double *loss_sum, int32_t *correct, int32_t *pred,
                                 int64_t ld_pred, int64_t K, int64_t C, void *scratch,
                                 int64_t scratch_bytes, void *stream);

/* Evaluation of GN-LeNet on the listed rows: the job model, the outputs and the contracts of
 * niidmix_linear_eval_rows_f32 for the reference's second model (setup/model/gn_lenet.py).  Job i
 * evaluates slab row rows[i] on the contiguous samples data[seg_start[i] .. seg_start[i] +
 * seg_len[i]); rows may repeat and segments may coincide; nothing in theta is written.
 *   theta     [*, ld_t] parameters (device); a row holds model.parameters() in registration order:
 *               conv1.w [32,Cin,5,5], conv1.b [32], gn1.w [32], gn1.b [32],
 *               conv2.w [32,32,5,5],  conv2.b [32], gn2.w [32], gn2.b [32],
 *               conv3.w [64,32,5,5],  conv3.b [64], gn3.w [64], gn3.b [64],
 *               fc.w [C,F], fc.b [C]
 *             with F = 64 h3 w3, h_{i+1} = floor((h_i - 3) / 2) + 1 three times from H (w from W);
 *             P = 800 Cin + 77184 + C F + C columns (80554 at Cin 1, 28 x 28 or 24 x 24, C 10;
 *             85354 at Cin 3, 32 x 32, C 10)
 *   data      [S, Cin * H * W] samples, each [Cin, H, W] row-major (device), labels [S] int32
 *   rows, seg_start, seg_len   [n_jobs] int32 (device); seg_len[i] is clamped to [0, max_len]
 *   loss_sum  [n_jobs] double (device): sum_s nll_s; each nll_s is fp32 and they are added in
 *             double, in sample order within a tile of 2 samples, the tiles in tile order
 *   correct   [n_jobs] int32 (device): #{s : pred_s == y_s}
 *   pred      NULL, or [n_jobs, ld_pred] int32 (device); entries at or past seg_len[i] untouched
 *   logits    NULL, or [n_jobs, ld_logits, C] fp32 (device): the classifier's output z (before
 *             log_softmax) of job i's j-th sample at (i * ld_logits + j) * C; entries at or past
 *             seg_len[i] untouched
 *   scratch   caller-owned device buffer (8-B aligned) of at least
 *             niidmix_gnlenet_eval_rows_scratch_bytes(n_jobs, max_len, Cin, H, W, C) bytes: per
 *             (job, tile) partial sums and counts and, when a tile's activations do not fit in LDS
 *             (H or W above 34 or so), activation slots for at most 4096 resident workgroups, so
 *             the size is bounded by a term proportional to the call's jobs plus a constant
 * The forward pass is the reference's:
 *   conv(5 x 5, stride 1, zero padding 2) -> maxpool(3, stride 2, floor) -> GroupNorm -> ReLU
 *   conv -> GroupNorm -> maxpool -> ReLU;  conv -> GroupNorm -> maxpool -> ReLU
 *   flatten in (channel, row, column) order -> linear
 * with 32 / 32 / 64 channels and GroupNorm(2 groups, eps 1e-5, biased variance, affine).  The
 * group statistics take two passes, the mean and then the centred squares, both fp32.  pred_s and
 * nll_s = lse(z_s) - z[s, y_s] follow niidmix_linear_eval_rows_f32's rule: the lowest index that
 * attains the maximum, a NaN counting as the maximum, the first NaN winning.  A job of length 0
 * gets 0.0 and 0.
 * fp32 FMAs only, every value a chain or a fixed tree of one workgroup; no floating-point atomics:
 * two calls on the same inputs give the same bits; a job's outputs depend neither on which other
 * jobs the call lists nor on how the caller splits the job list over calls; theta is not written;
 * an inf or NaN in one row's parameters stays in the jobs that list that row.  Not bit-identical to
 * ATen's CPU result (another summation order): the logits are within 4 e32 of the float64 forward,
 * e32 being the error of torch's own fp32 forward on the CPU (tests/test_gpu_eval_gnlenet.py).
 * Limits (NIIDMIX_EUNSUPPORTED beyond): C <= 1024, Cin <= 4, 15 <= H, W <= 64 (below 15 the third
 * pool has no output).  Any ld_t >= P, any alignment of theta and data.
 * Checked before anything touches the GPU, in this order:
 *   NIIDMIX_EINVAL        a null pointer other than pred and logits
 *   NIIDMIX_EINVAL        n_jobs, Cin, H, W or C < 1, max_len < 0
 *   NIIDMIX_EUNSUPPORTED  C > 1024, Cin > 4, H or W outside [15, 64]
 *   NIIDMIX_EINVAL        ld_t < P
 *   NIIDMIX_EINVAL        ld_pred < max_len (pred given), ld_logits < max_len (logits given)
 *   NIIDMIX_EINVAL        a scratch buffer that is too small or not 8-B aligned
 *   NIIDMIX_EALIAS        loss_sum, correct, pred, logits or scratch overlaps theta (one row of
 *                         theta, P elements from its base, as for niidmix_linear_eval_rows_f32)
 * rows, seg_start, seg_len and labels are device data and are NOT checked by the launcher: a row
 * or a segment outside its array reads out of bounds (a label outside [0, C) matches no class).
 * niidmix.evaluate.DeviceEvaluator checks them and builds the job lists itself. */
int64_t niidmix_gnlenet_eval_rows_scratch_bytes(int64_t n_jobs, int64_t max_len, int64_t Cin,
                                                int64_t H, int64_t W, int64_t C);
int niidmix_gnlenet_eval_rows_f32(const float *theta, int64_t ld_t, const float *data,
                                  const int32_t *labels, const int32_t *rows,
                                  const int32_t *seg_start, const int32_t *seg_len, int64_t n_jobs,
                                  int64_t max_len, double *loss_sum, int32_t *correct, int32_t *pred,
                                  int64_t ld_pred, float *logits, int64_t ld_logits, int64_t Cin,
                                  int64_t H, int64_t W, int64_t C, void *scratch,
                                  int64_t scratch_bytes, void *stream);

/* Local training of GN-LeNet on the listed rows: gradient and loss of one mini-batch per row, for
 * every row in one call (the drop-in's --device-training-gn-lenet; niidmix.train.DeviceTrainer).
 * The job model and the argument meanings are those of niidmix_linear_nll_grad_rows_f32; the row
 * layout, the data layout, the limits and the forward pass are those of
 * niidmix_gnlenet_eval_rows_f32.
 *   theta     [*, ld_t] parameters (device): a row holds the model's 14 tensors, P columns
 *   data      [S, Cin * H * W] samples, each [Cin, H, W] row-major (device), labels [S] int32
 *   batch_idx [n_rows, b_max] int32 sample indices into data (device); entry i belongs to rows[i]
 *   batch_len [n_rows] int32 (device), clamped to [0, b_max]: entries past len are not read.  A
 *             length of 0 gives a zero gradient and a NaN loss (0 / 0, as F.nll_loss of no samples)
 *   rows      [n_rows] int32 distinct slab rows (device)
 *   grad      [*, ld_g] gradients (device), row layout of theta: all P elements of a listed row are
 *             written, other rows and columns past P are untouched
 *   loss      [n_rows] mean batch loss of rows[i] (device)
 *   scratch   caller-owned device buffer (8-B aligned) of at least
 *             niidmix_gnlenet_nll_grad_rows_scratch_bytes(n_rows, b_max, Cin, H, W, C) bytes: a
 *             slot per (row, tile of 2 samples) with every activation the backward pass needs and
 *             the sample's gradients, so the size is proportional to n_rows * ceil(b_max / 2)
 *             (about 184 KB per sample at 3 x 32 x 32, 130 KB at 1 x 28 x 28); its contents are
 *             overwritten
 * The result is that of F.nll_loss(model.forward(x), y).backward() on a zeroed gradient:
 *   softmax    dz[s,c] = (exp(z[s,c] - lse_s) - [c == y_s]) / len,  loss = (1/len) sum_s (lse_s - z[s,y_s])
 *   linear     dW[c,f] = sum_s dz[s,c] feat[s,f],  db[c] = sum_s dz[s,c],  dfeat = dz W
 *   ReLU       the gradient passes where the output is > 0
 *   max-pool   (3, stride 2) the gradient of a window goes to its first maximum in (row, column)
 *              scan order, a NaN counting as a maximum (the forward's and torch's rule).  Windows
 *              overlap: every source position gathers from the at most 4 windows that cover it.
 *   GroupNorm  (2 groups, eps 1e-5, biased variance) per (sample, group) of n elements, with
 *              xh = (x - mean) rstd and gh = dout gamma_c:  dx = rstd (gh - mean(gh) - xh mean(gh xh)),
 *              dgamma_c = sum dout xh,  dbeta_c = sum dout
 *   conv       (5 x 5, zero padding 2) weight, bias and data gradients; conv1 has no data gradient
 *              and its weight gradient reads the input at the first pool's argmax positions
 * fp32 FMAs only and no floating-point atomics.  Every weight gradient is one fma chain per sample
 * over the at most h w positions of its map, the samples then added in batch order; the sums of
 * GroupNorm are fixed trees of one wave.  Two calls on the same inputs give the same bits; a row's
 * grad and loss bits depend neither on which other rows the call lists nor on how the caller
 * splits the row list over calls; theta is not written; an inf or NaN in one row's parameters stays
 * in that row's outputs.  Not bit-identical to ATen's CPU result (another summation order): every
 * tensor's gradient is within 4 e32 of the float64 gradient relative to that tensor's largest
 * element, e32 being the same measure of torch's own fp32 autograd on the CPU
 * (tests/test_gpu_train_gnlenet.py).
 * Limits (NIIDMIX_EUNSUPPORTED beyond): C <= 1024, Cin <= 4, 15 <= H, W <= 64, b_max <= 2^24,
 * n_rows <= 2^24, n_rows * ceil(b_max / 2) < 2^31 scratch slots (the scratch size then stays far
 * inside int64; the size function returns 0 beyond), n_rows * ceil((C F + C) / 256) < 2^31 blocks.
 * Any ld_t, ld_g >= P, any alignment of theta, grad and data.
 * Checked before anything touches the GPU, in this order:
 *   NIIDMIX_EINVAL        a null pointer
 *   NIIDMIX_EINVAL        n_rows, b_max, Cin, H, W or C < 1
 *   NIIDMIX_EUNSUPPORTED  C > 1024, Cin > 4, H or W outside [15, 64], b_max or n_rows too large
 *   NIIDMIX_EINVAL        ld_t < P or ld_g < P
 *   NIIDMIX_EINVAL        a scratch buffer that is too small or not 8-B aligned
 *   NIIDMIX_EALIAS        grad, loss or scratch overlaps theta, or grad overlaps scratch, theta and
 *                         grad taken over the least extent n_rows distinct rows can span,
 *                         (n_rows - 1) * ld + P elements (the row list is on the device and is not
 *                         read by the launcher)
 * batch_idx, batch_len, labels and rows are device data and are NOT checked by the launcher: an
 * index outside data reads out of bounds (a label outside [0, C) matches no class).
 * niidmix.train.DeviceTrainer checks them once per node set. */
int64_t niidmix_gnlenet_nll_grad_rows_scratch_bytes(int64_t n_rows, int64_t b_max, int64_t Cin,
                                                    int64_t H, int64_t W, int64_t C);
int niidmix_gnlenet_nll_grad_rows_f32(const float *theta, int64_t ld_t, const float *data,
                                      const int32_t *labels, const int32_t *batch_idx,
                                      const int32_t *batch_len, int64_t b_max, const int32_t *rows,
                                      int64_t n_rows, float *grad, int64_t ld_g, float *loss,
                                      int64_t Cin, int64_t H, int64_t W, int64_t C, void *scratch,
                                      int64_t scratch_bytes, void *stream);

/* Training batches drawn on the device (the drop-in's --device-sampling): job j writes the batch
 * that starts at position cursor[j] of epoch epoch[j]'s permutation of the segment
 * [seg_start[j], seg_start[j] + seg_len[j]) of the caller's concatenated data, in the layout
 * niidmix_linear_nll_grad_rows_f32 and niidmix_gnlenet_nll_grad_rows_f32 read:
 *     batch_len[j]     = min(b_max, seg_len[j] - cursor[j])
 *     batch_idx[j, t]  = seg_start[j] + perm[cursor[j] + t]      for 0 <= t < batch_len[j]
 * entries past batch_len[j] are untouched.  The permutation is a stream of this library's own,
 * defined in integers (niidmix/sampling.py restates it in numpy; the two agree exactly): position
 * i of the segment gets the 32-bit key
 *     k_i = word (i & 3) of Philox4x32-10(counter (i >> 2, epoch[j], 0, 0), key (seed, rank[j]))
 * (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85), and perm lists the
 * positions in ascending order of the 64-bit composites (k_i << 32) | i, which are distinct.
 *   seed      the run's seed, low 32 bits
 *   rank, seg_start, seg_len, epoch, cursor   [n_jobs] int32 (device); ranks may come in any order
 *             and segments may coincide
 *   batch_idx [n_jobs, b_max] int32 (device), batch_len [n_jobs] int32 (device)
 * The call is stateless: one workgroup per job sorts the whole segment every time (in registers
 * of one wave up to 64 samples, else in LDS), so two calls on the same inputs give the same bits.
 * niidmix_draw_batches_max_len() is the longest segment a workgroup sorts (8192: composites of 8 B
 * in 64 KiB of LDS).  The per-job arrays are device data and are NOT read by the launcher: the
 * kernel clamps a longer seg_len to the maximum (the permutation is then that of the clamped
 * length; niidmix.train refuses such a node list) and writes batch_len 0 and no index for a cursor
 * outside [0, seg_len) -- nothing is read or written out of range.
 * Checked before anything touches the GPU, in this order:
 *   NIIDMIX_EINVAL        a null pointer
 *   NIIDMIX_EINVAL        n_jobs or b_max < 1
 *   NIIDMIX_EUNSUPPORTED  b_max above niidmix_draw_batches_max_len(), n_jobs >= 2^31
 *   NIIDMIX_EALIAS        batch_idx or batch_len overlaps an input or the other output
 * A pure addition: the ABI version is unchanged. */
int64_t niidmix_draw_batches_max_len(void);
int niidmix_draw_batches_i32(uint32_t seed, const int32_t *rank, const int32_t *seg_start,
                             const int32_t *seg_len, const int32_t *epoch, const int32_t *cursor,
                             int64_t n_jobs, int64_t b_max, int32_t *batch_idx, int32_t *batch_len,
                             void *stream);

/* The same stream, sorted once per epoch and kept (the drop-in's --device-sampling-cached, for
 * train-sets longer than one workgroup sorts): niidmix_epoch_perm_i32 writes job j's whole
 * permutation of epoch[j] -- seg_len[j] segment-local positions, the ascending order of the
 * composites above -- to perm[perm_off[j] .. perm_off[j] + seg_len[j]), and
 * niidmix_take_batches_i32 slices such a cache every round, in niidmix_draw_batches_i32's layout:
 *     batch_len[j]     = min(b_max, seg_len[j] - cursor[j])
 *     batch_idx[j, t]  = seg_start[j] + perm[perm_off[j] + cursor[j] + t]   for 0 <= t < batch_len[j]
 * For segments of at most niidmix_draw_batches_max_len() samples the two calls give, bit for bit,
 * what niidmix_draw_batches_i32 gives on the same jobs.
 *   rank, seg_len, epoch, seg_start, cursor   [n_jobs] int32 (device)
 *   perm_off  [n_jobs] int64 (device): the jobs' stretches of perm; they must not overlap each
 *             other (not checked: overlapping stretches have two writers)
 *   perm      [perm_len] int32 (device)
 *   max_len   (host) the longest seg_len among the jobs: the launcher sizes its grid and the
 *             scratch by it without reading device memory.  The kernels clamp a longer seg_len to
 *             it (the permutation is then that of the clamped length).
 *   scratch   (device, 16-B aligned) niidmix_epoch_perm_scratch_bytes(n_jobs, max_len) bytes: 0
 *             (scratch may be NULL) when max_len <= niidmix_draw_batches_max_len(), else
 *             n_jobs * pow2(max_len) * 8, pow2 the next power of two
 * Segments up to niidmix_draw_batches_max_len() are sorted by one workgroup in LDS, as there.  A
 * longer one is one bitonic network over pow2(seg_len) composites in the scratch (all-ones
 * padding): a workgroup sorts each chunk of 8192 in LDS, then every level takes one launch per
 * stage of stride >= 8192 in global memory and one launch that finishes it in LDS.  Every word
 * has one writer and no stage depends on scheduling: two calls give the same bits.
 * niidmix_epoch_perm_max_len() is the longest segment (2^20 = 1048576: 36 launches).
 * The per-job arrays are device data and are NOT read by the launcher.  A job whose stretch
 * [perm_off, perm_off + seg_len) does not lie inside [0, perm_len) is skipped by
 * niidmix_epoch_perm_i32 and gets batch_len 0 from niidmix_take_batches_i32, as does a cursor
 * outside [0, seg_len); slots past batch_len are untouched -- nothing is read or written out of
 * range whatever the arrays hold.
 * Checked before anything touches the GPU, in this order:
 *   NIIDMIX_EINVAL        a null pointer (scratch only when max_len needs one)
 *   NIIDMIX_EINVAL        n_jobs, max_len, b_max or perm_len < 1
 *   NIIDMIX_EUNSUPPORTED  max_len or b_max above niidmix_epoch_perm_max_len(), n_jobs >= 2^31
 *   NIIDMIX_EINVAL        scratch_bytes below the need, scratch not 16-B aligned
 *   NIIDMIX_EALIAS        an output (perm, scratch; batch_idx, batch_len) overlaps an input or the
 *                         other output
 * Pure additions: the ABI version is unchanged. */
int64_t niidmix_epoch_perm_max_len(void);
int64_t niidmix_epoch_perm_scratch_bytes(int64_t n_jobs, int64_t max_len);
int niidmix_epoch_perm_i32(uint32_t seed, const int32_t *rank, const int32_t *seg_len, const int32_t *epoch,
                           const int64_t *perm_off, int64_t n_jobs, int64_t max_len, int32_t *perm,
                           int64_t perm_len, void *scratch, int64_t scratch_bytes, void *stream);
int niidmix_take_batches_i32(const int32_t *perm, int64_t perm_len, const int64_t *perm_off,
                             const int32_t *seg_start, const int32_t *seg_len, const int32_t *cursor,
                             int64_t n_jobs, int64_t b_max, int32_t *batch_idx, int32_t *batch_len,
                             void *stream);

/* torch's own permutations for the same cache (the drop-in's --device-sampling-torch-stream: the
 * batches of the CPU path's DataLoaders, shuffled on the device): job j writes to
 * perm[perm_off[j] .. perm_off[j] + seg_len[j]) the permutation that
 *     torch.randperm(seg_len[j], generator=g)      after g.manual_seed(s), on the CPU
 * gives for every s whose low 32 bits are seed_lo[j] (the int32 read as uint32), in
 * niidmix_epoch_perm_i32's index convention (segment-local positions), so niidmix_take_batches_i32
 * slices it unchanged.  That is MT19937 seeded by init_genrand(seed_lo[j]) feeding
 *     for i in 0 .. seg_len-2:  z = next_u32 % (seg_len - i);  swap(a[i], a[i + z])
 * on a = 0 .. seg_len-1 (niidmix/sampling.py, torch_permutation, restates it in numpy).
 *   seed_lo, seg_len   [n_jobs] int32 (device)
 *   perm_off  [n_jobs] int64 (device): the jobs' stretches of perm; they must not overlap each
 *             other (not checked: overlapping stretches have two writers)
 *   perm      [perm_len] int32 (device)
 *   max_len   (host) the longest seg_len among the jobs: it sizes the workgroups' LDS
 *             (2 * max_len + 3744 bytes, rounded up to 16)
 * One workgroup per job keeps the positions as uint16 in LDS, so
 * niidmix_torch_randperm_max_len() is 65536; the swaps are walked by one lane (the chain is
 * serial), everything else by the workgroup.  No scratch.  Every word has one writer: two calls
 * give the same bits.
 * The per-job arrays are device data and are NOT read by the launcher.  A job whose seg_len is
 * outside 1..max_len, or whose stretch does not lie inside [0, perm_len), is skipped and writes
 * nothing -- nothing is read or written out of range whatever the arrays hold.
 * Checked before anything touches the GPU, in this order:
 *   NIIDMIX_EINVAL        a null pointer
 *   NIIDMIX_EINVAL        n_jobs, max_len or perm_len < 1
 *   NIIDMIX_EUNSUPPORTED  max_len above niidmix_torch_randperm_max_len(), n_jobs >= 2^31
 *   NIIDMIX_EALIAS        perm overlaps an input
 * Pure additions: the ABI version is unchanged. */
int64_t niidmix_torch_randperm_max_len(void);
int niidmix_torch_randperm_i32(const int32_t *seed_lo, const int32_t *seg_len, const int64_t *perm_off,
                               int64_t n_jobs, int64_t max_len, int32_t *perm, int64_t perm_len,
                               void *stream);

/* update_models(all_models, avg) after the 'sample' topology's uniform average (d_sgd.py:240-250,
 * :29-35): every row y_i := fl(fl(x_i * 0) + avg) (p.mul_(0.); p.add_(new)) — avg everywhere
 * except NaN where x_i is non-finite and the sign rule of (+-0) + (+-0) where avg is 0.
 *   x [n_rows, ld_x], y [n_rows, ld_y] (device; y == x with ld_y == ld_x: in place, any other
 *   overlap is refused);  avg [p] (device, overlapping neither) */
int niidmix_update_rows_f32(const float *x, int64_t ld_x, float *y, int64_t ld_y, int64_t n_rows,
                            int64_t p, const float *avg, void *stream);

/* Sharded round over several GPUs of ONE process (the simulator's own model: every node in one
 * process, run.py:136), nodes sharded by whole cliques (niidmix.shard.ShardPlan), the rows other
 * shards read exchanged every round, then each shard's rows mixed by niidmix_mix_csr_f32 over
 * [local rows | halo rows] (the local CSR keeps every row's operand order: exact mode is bitwise
 * the single-GPU round).  The handle holds one RCCL communicator per shard (ncclCommInitAll,
 * created once per topology and device set; librccl.so.1 is loaded on first use).  When several
 * shards share a device (tests, one-GPU boxes) the exchange is device-to-device copies instead.
 * Shard s, row-major slabs with ld = p:
 *   x [rows_in, p]: its n_local rows, then its halo rows;  y [n_local, p]
 *   row_ptr / col / val: CSR of its n_local rows over the rows_in input rows (device)
 *   peer[j], j < n_peers (host): the shards it exchanges with; it sends
 *     send_rows[send_ptr[j] .. send_ptr[j+1]) (device local row indices, in that peer's halo order;
 *     send_ptr host, send_ptr[0] may be > 0) through send_buf (device, [send_ptr[n_peers] -
 *     send_ptr[0], p]) and receives recv_count[j] rows into halo rows recv_row[j] .. (host)
 *   stream: the shard's HIP stream (on its device)
 * Every shard's receive count must equal what the peer sends it (checked); the call enqueues
 * pack -> exchange -> mix on every shard's stream and returns without waiting. */
typedef struct niidmix_sharded niidmix_sharded;
typedef struct niidmix_shard {
    int32_t device;
    int32_t n_peers;
    int64_t n_local, rows_in;
    float *x;
    float *y;
    const int64_t *row_ptr;
    const int32_t *col;
    const float *val;
    const int32_t *peer;
    const int64_t *send_ptr;
    const int32_t *send_rows;
    float *send_buf;
    const int64_t *recv_row;
    const int64_t *recv_count;
    void *stream;
} niidmix_shard;

int niidmix_sharded_create(int n_shards, const int *devices, niidmix_sharded **out);
int niidmix_sharded_destroy(niidmix_sharded *h);
/* 1 when the handle exchanges by device-to-device copies (shards sharing a device), 0 for RCCL. */
int niidmix_sharded_is_loopback(const niidmix_sharded *h);
int niidmix_mix_sharded_f32(niidmix_sharded *h, const niidmix_shard *shards, int64_t p, int mode);

/* Device memory for node-state slabs, with the signatures of a PyTorch pluggable allocator
 * (torch.cuda.memory.CUDAPluggableAllocator; niidmix.memory.slab_pool uses them for a MemPool).
 * The range is reserved with hipMemAddressReserve and mapped from 2 MiB physical chunks
 * (hipMemCreate / hipMemMap): the clique kernel's access pattern measured 1.32 ms per headline round
 * on every such slab, against 1.35-1.64 ms on hipMalloc'ed slabs depending on their physical
 * placement.  Returns NULL on failure (niidmix_last_error says why); free with
 * niidmix_hbm_free (size, device and stream are ignored). */
void *niidmix_hbm_alloc(ssize_t size, int device, void *stream);
void niidmix_hbm_free(void *ptr, ssize_t size, int device, void *stream);

/* Strided host <-> device copy (hipMemcpy2DAsync) of `rows` rows of `width_bytes` each, used by
 * the host-resident drop-in (niidmix.slab) to stream column windows of the pinned [N, P] host slab
 * through HBM while the previous window is being mixed.  kind: 0 = host->device, 1 = device->host,
 * 2 = device->device.  Stream-ordered; host memory must be pinned for the copy to be asynchronous. */
int niidmix_copy2d_async(void *dst, int64_t dpitch_bytes, const void *src, int64_t spitch_bytes,
                         int64_t width_bytes, int64_t rows, int kind, void *stream);

/* Streaming copy y[0:n] = x[0:n] (fp32, n % 4 == 0, 16-B aligned, no overlap) with non-temporal
 * loads and stores, one float4 per thread in linear order.  Not part of the reference's path: a
 * measurement primitive that gives bench.py this GPU's own HBM copy ceiling to report the mixing
 * kernel against (MI355X boxes differ by up to ~20 % in achievable HBM bandwidth). */
int niidmix_stream_copy_f32(const float *x, float *y, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* NIIDMIX_H */
