/* dba_hip.h -- C ABI of the MI355X (gfx950) dense-bundle-adjustment / correlation backend.
 *
 * This is the drop-in boundary of the hot path: plain pointers, sizes and a HIP stream; no
 * torch types.  Every entry point names the reference interface it replaces
 * (paths relative to GREAT-WHU/DBA-Fusion, i.e. /root/reference).  The reference binds these
 * operations through the pybind11 module `droid_backends` (src/droid.cpp:297-316); the module of
 * the same name under dba-fusion_amd/droid_backends/ is a thin adapter over this ABI
 * (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Conventions
 *   - all data pointers are DEVICE pointers unless the parameter name ends in _host;
 *   - tensors are dense row-major ("contiguous"), shapes given in comments;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued, never synchronised,
 *     unless stated otherwise; results are visible to later work on the same stream;
 *   - return value: 0 = DBA_OK, negative = error (see enum); numerical failure of the pose
 *     solve is NOT an error: like the reference it yields a zero update
 *     (src/droid_kernels.cu:193-196, :1263-1266).
 */
#ifndef DBA_HIP_H
#define DBA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  DBA_OK = 0,
  DBA_ERR_ARG = -1,       /* bad size / null pointer */
  DBA_ERR_WORKSPACE = -2, /* workspace too small */
  DBA_ERR_HIP = -3,       /* a HIP runtime call failed (see dba_last_error) */
  DBA_ERR_UNSUPPORTED = -4
};

enum { DBA_F32 = 0, DBA_F16 = 1, DBA_F64 = 2, DBA_U8 = 3 }; /* element type selector for volume/corr buffers; DBA_U8 only as dba_enc_image's src_dtype */

typedef void *dba_stream_t;

const char *dba_version(void);
const char *dba_last_error(void); /* text of the last DBA_ERR_HIP on this thread */

/* ------------------------------------------------------------------------------------------
 * Dense bundle adjustment: droid_backends.ba  (src/droid.cpp:109-138 -> ba_cuda,
 * src/droid_kernels.cu:1394-1512) and class BACore (src/bacore.h:4-70,
 * src/droid_kernels.cu:1786-1956).
 *
 *   poses       [B,7]   f32 (tx,ty,tz,qx,qy,qz,qw) world->camera; rows [t0,t1) updated in place
 *   disps       [B,ht,wd] f32 inverse depth; rows kx = unique(arange(t0,t1) U ii) updated in place
 *   intrinsics  [4]     f32 (fx,fy,cx,cy) at 1/8 resolution
 *   disps_sens  [B,ht,wd] f32, 0 = no depth measurement
 *   targets, weights [N,2,ht,wd] f32 (ch0 = x/u, ch1 = y/v)
 *   eta         [eta_rows,ht,wd] f32, eta_rows == |kx| or 1 (broadcast)
 *   ii, jj      [N] int64 on the device
 *   frame_owned [B] uint8 or NULL: multi-GPU edge sharding by source frame -- a rank linearises
 *               the edges it was given and updates depth only for frames it owns (NULL = all)
 *
 * The workspace (device memory, dba_ba_workspace_bytes) holds the index tables, the
 * depth/pose coupling rows E, Q = 1/C, w, the reduced camera system (float64) and dx.
 * ---------------------------------------------------------------------------------------- */

size_t dba_ba_workspace_bytes(int N, int B, int ht, int wd, int t0, int t1);

/* byte offsets inside the workspace of the pieces a host may need to touch between stages
 * (multi-GPU all-reduce of H/b; BACore handing H/v to the caller).  H is [6P,6P] float64 row-major,
 * b is [6P] float64, dx is [P,6] float32, meta[0] = |kx| (int32), meta[1] = 1 if the last solve failed. */
typedef struct {
  size_t H, b, dx, meta, E, Q, w, kx;
  int P, Mmax, nchunks;
} dba_ba_layout;
int dba_ba_get_layout(int N, int B, int ht, int wd, int t0, int t1, dba_ba_layout *out);

/* stage 0: index sets on the device (replaces the per-iteration host bookkeeping of
 * ba_cuda :1416-1424, accum_cuda :993-1043 and schur_block :1307-1347). */
int dba_ba_prepare(const int64_t *ii, const int64_t *jj, int N, int B, int ht, int wd, int t0, int t1,
                   void *ws, size_t ws_bytes, dba_stream_t stream);
/* Stage 0 keyed on the CONTENTS of the edge list.  The reference's caller hands droid_backends.ba new ii / jj tensors with
 * the same edges on every update (torch.cat with the inactive edges, dbaf/covisible_graph.py:242-247), so "same graph as
 * last time" cannot be decided on tensor identity.  Stage 0 leaves a key in the workspace (N, B, t0, t1, Schur form, ii, jj);
 * check != 0: the launch compares the call's edge list with that key on the device and returns at once when the tables
 * are those of this graph already (no host synchronisation either way).  check != 0 needs a workspace whose key area is
 * valid: one that went through dba_ba_workspace_init (fresh memory) or an earlier stage 0.
 * eta_rows > 1: the number of rows of the call's eta, which must equal |kx| (droid_kernels.cu:1476 adds eta.view(-1, HW) to
 * the |kx| rows of C; the reference raises a broadcast error otherwise).  |kx| only exists on the device, so a mismatch is
 * recorded in pinned host memory and reported by dba_ba_poll_eta_error[_ws]; the call it belongs to changes nothing. */
int dba_ba_prepare_keyed(const int64_t *ii, const int64_t *jj, int N, int B, int ht, int wd, int t0, int t1, int eta_rows,
                         int check, void *ws, size_t ws_bytes, dba_stream_t stream);
/* diagnostic: what the library currently believes about the reduced camera system of this workspace's graph -- 1: banded enough
 * for the window solver (csrc/ba_solve_wave.hip), 2: not (the register-tile / skyline / general kernels serve it), 0: nothing
 * known yet; negative: error.  Host memory only, no synchronisation: the value is written by stage 0 when it rebuilds a graph's
 * tables inside dba_ba / dba_ba_run and by the window solver itself, and steers where the NEXT solves of the workspace are sent
 * (only ever a hint: every kernel solves whatever it is given).  Replaces the host-side choice of Eigen::LLT / SimplicialLLT
 * by matrix size in /root/reference/src/droid_kernels.cu:200-218,1248-1269. */
int dba_ba_solver_verdict(int N, int B, int ht, int wd, int t0, int t1, void *ws, size_t ws_bytes);
/* marks a freshly allocated workspace as "no graph prepared" (clears meta and the key header; asynchronous on `stream`) */
int dba_ba_workspace_init(int N, int B, int ht, int wd, int t0, int t1, void *ws, size_t ws_bytes, dba_stream_t stream);
/* 1 (and the two counts) if a stage 0 that has COMPLETED since the last poll saw eta_rows != |kx| on any workspace, else 0; clears
 * that record.
 * Host memory only: no synchronisation.  The adapters poll at the top of every ba call and raise for the earlier one. */
int dba_ba_poll_eta_error(int *eta_rows, int *num_kx);
/* the same for ONE workspace (the report lives in pinned words of the workspace stage 0 ran on, so a mismatch is attributed to the
 * caller that made it whatever other devices, streams or threads do).  The offending call itself is harmless: stage 0 also leaves
 * its verdict in the workspace, and the kernels that write the caller's state honour it -- poses and inverse depths stay as they
 * were, dx and dz come back zero (the reference raises before it touches anything: /root/reference/src/droid_kernels.cu:1476). */
int dba_ba_poll_eta_error_ws(int N, int B, int ht, int wd, int t0, int t1, void *ws, size_t ws_bytes, int *eta_rows, int *num_kx);

/* The edge tensors of one BA call as the reference's caller assembles them (dbaf/covisible_graph.py:242-247: torch.cat of the
 * selected inactive edges' and the active edges' ii / jj / target / weight; :332-333: target, weight from [n, ht, wd, 2] to the
 * planar [n, 2, ht, wd] of the binding droid.cpp:301) in one launch instead of ten.  target_* / weight_*: [n_*, ht, wd, 2]
 * float32; sel: n_sel indices into the inactive list (int64, device; null: its first n_sel edges); outputs: targets_out,
 * weights_out [n_sel + n_act, 2, ht, wd], ii_out, jj_out [n_sel + n_act] -- the arguments of dba_ba / droid_backends.ba. */
int dba_ba_gather_edges(const float *target_inac, const float *weight_inac, const int64_t *ii_inac, const int64_t *jj_inac,
                        int n_inac, const int64_t *sel, int n_sel, const float *target_act, const float *weight_act,
                        const int64_t *ii_act, const int64_t *jj_act, int n_act, int ht, int wd, float *targets_out,
                        float *weights_out, int64_t *ii_out, int64_t *jj_out, dba_stream_t stream);

/* stage 1: fused per-source-frame linearisation (projective_transform_kernel :220-468 +
 * accum_kernel :899-919 + C/w/Q assembly :1474-1478); also clears H, b.  alpha = 0.05 for
 * droid_backends.ba (:1474), 0.001 for BACore::hessian (:1872). */
int dba_ba_linearize(const float *poses, const float *disps, const float *intrinsics,
                     const float *disps_sens, const float *targets, const float *weights,
                     const float *eta, int eta_rows, const int64_t *ii, const int64_t *jj,
                     const uint8_t *frame_owned, int N, int B, int ht, int wd, int t0, int t1,
                     float alpha, void *ws, size_t ws_bytes, dba_stream_t stream);

/* stage 2: reduced camera system  H = A - E Q E^T,  b = v - E Q w  in float64
 * (SparseBlock::update_lhs/rhs :1176-1218, schur_block + EEt6x6/Ev6x1 :1046-1138, :1297-1391).
 * motion_only != 0 assembles A, v alone (:1464-1471). */
int dba_ba_reduce(const int64_t *ii, const int64_t *jj, const uint8_t *frame_owned, int N, int B,
                  int ht, int wd, int t0, int t1, int motion_only, void *ws, size_t ws_bytes,
                  dba_stream_t stream);

/* Which kernel forms the Schur products of stage 2 (must be set before dba_ba_prepare of the call it applies to: the
 * prepare stage builds the tables of the form in force): 0 = automatic (the per-source-frame form -- float64 Gram tiles on
 * the matrix cores, every row of E read once -- on windows whose frames couple many rows, the (row, partner) grid on
 * sparse ones), 1 = (row, partner) grid, 2 = per-source-frame form.  Initialised from DBA_SCHUR_KERNEL = rows | frame. */
int dba_ba_schur_select(int form);
int dba_ba_schur_select_thread(int form); /* the same choice for the calling host thread only (0 = none); the process-wide
                                           * dba_ba_schur_select wins when both are set */
int dba_ba_schur_thread_form(void);        /* the calling thread's pin (0 = none): part of the key of a prepared workspace */
int dba_ba_schur_auto_form(int N, int P); /* the form (1 or 2) the automatic choice gives a graph of N edges over a window of
                                           * P optimised poses (rows per source frame ~ 1 + N / (P + 1); a function of the
                                           * graph, not of the video buffer's size): the sharded driver asks with the
                                           * COMPLETE graph's numbers and pins that form on every rank for the duration of
                                           * the call (a rank's share has the same rows per frame, but few edges) */
int dba_ba_schur_generation(void); /* number of dba_ba_schur_select calls so far: tables prepared under another generation
                                    * may lack what the form in force needs (callers of dba_ba_prepared compare it) */
/* How the (row, partner) form walks its pairs: 0 = one workgroup per pair of the list stage 0 leaves in the workspace, with a
 * chunk's pixels loaded in one phase and one transposing reduction per wave; 1 = the (row, partner slot) grid.  Both form the
 * same sums (bit for bit in deterministic mode) and read the same tables, so the switch may change between any two calls.
 * Initialised from DBA_SCHUR_SPARSE = legacy. */
int dba_ba_schur_sparse_select(int legacy);
/* where that list lies in the workspace (bytes from its start) and how many pairs it holds at most: int32 [1 + capacity][4],
 * entry 0 = {number of pairs or -1 (not listed), 0, 0, 0}, entry 1 + i = {row r1, row r2, tgt1 | tgt2 << 16, slot} */
int dba_ba_pairs_table(int N, int B, int ht, int wd, int t0, int t1, size_t *offset, int *capacity);

/* Deterministic accumulation of H, b (off by default; DBA_DETERMINISTIC=1 turns it on at load).  The reference adds the
 * blocks of the camera system on the host in a fixed order (SparseBlock::update_lhs / update_rhs, droid_kernels.cu:1176-1218);
 * this path adds them with float64 atomics from many workgroups, which is order-dependent in the last bits.  With the mode
 * on every addend is rounded once to a multiple of 2^-30 and summed with 64-bit integer atomics (associative): H, b, and
 * with them dx and the retracted state, are identical bit for bit from run to run and between a single GPU and any number
 * of ranks.  Costs one small launch per Gauss-Newton iteration. */
int dba_ba_set_deterministic(int on);

/* opt-in guard (also DBA_SOLVE_CHECK=1): behind every solve a kernel checks the residual of the damped system at the float
 * solution; a solve that is wrong beyond rounding becomes a zero update with the failure flag set, as a failed factorisation
 * does (/root/reference/src/droid_kernels.cu:1263-1266).  ~5 us per solve; off by default: the solvers' flag protocols are covered
 * by the cold-start stress of the GPU suite (tests/test_gpu_solve_cold.py). */
int dba_ba_set_solve_check(int on);
/* the check alone, on what lies in the workspace (H lower triangle, b, dx) */
int dba_ba_solve_check(int N, int B, int ht, int wd, int t0, int t1, float lm, float ep, void *ws, size_t ws_bytes,
                       dba_stream_t stream);

/* H <- its lower triangle mirrored.  dba_ba and the sharded front stage keep only the lower triangle of H up (what the
 * solvers read: half the float64 atomics); a caller that hands the full matrix on (ShardedBACore.hessian -> GTSAM) mirrors it
 * first.  dba_ba_reduce and dba_bacore_hessian always produce the full matrix (mirrored from the lower triangle: symmetric
 * to the last bit). */
int dba_ba_symmetrize(int N, int B, int ht, int wd, int t0, int t1, void *ws, size_t ws_bytes, dba_stream_t stream);

/* stage 3: damped dense solve in float64 on the device
 * (SparseBlock::solve :1248-1269: diag += ep + lm*diag; LL^T; zeros on failure) -> dx.  With a skyline table: the five-wave
 * window kernel for banded systems up to 64 poses (csrc/ba_solve_wave.hip).  Otherwise / for other structures: register-tile
 * block LDL^T up to 29 poses, skyline variants up to 64 poses, blocked Cholesky beyond / for wide skylines (csrc/ba_solve*.hip).
 * This stage measures the skyline from H (the system may have been summed over ranks); dba_ba takes it from the
 * prepare stage's graph tables. */
int dba_ba_solve(int N, int B, int ht, int wd, int t0, int t1, float lm, float ep, void *ws,
                 size_t ws_bytes, dba_stream_t stream);
/* the same with the caller's pose-level skyline (device, t1 - t0 ints: for every pose the first pose it is coupled with, as
 * dba_ba_shard_back's window_fpose): what dba_ba hands the solvers from its graph tables.  With a skyline, banded systems
 * (every column inside the 48-row window of its 16-column tile: ~4 poses wide) go to the five-wave window kernel
 * (csrc/ba_solve_wave.hip); a system that turns out not to be banded is solved by the general kernel's code in the same
 * launch, and the next solve on this workspace goes to the register-tile / skyline kernels directly. */
int dba_ba_solve_skyline(int N, int B, int ht, int wd, int t0, int t1, float lm, float ep, const int32_t *fpose, void *ws,
                         size_t ws_bytes, dba_stream_t stream);

/* stage 4: back-substitution + retraction (EvT6x1_kernel :1140-1160, dz :1495,
 * pose_retr_kernel :943-976, disp_retr_kernel :978-991).  dz_out [>=|kx|, ht*wd] may be NULL.
 * update_poses / update_disps select which retractions are applied. */
int dba_ba_update(float *poses, float *disps, const int64_t *ii, const int64_t *jj,
                  const uint8_t *frame_owned, int N, int B, int ht, int wd, int t0, int t1,
                  int update_poses, int update_disps, float *dz_out, void *ws, size_t ws_bytes,
                  dba_stream_t stream);

/* The two halves of one Gauss-Newton iteration of a rank of the edge-sharded driver (dbaf_amd/sharded.py), one call
 * each: front = stages 1 + 2 on the rank's edges (its partial [H | b] is then summed over the ranks by the caller: one
 * RCCL all-reduce), back = stages 3 + 4 on the summed system (every rank solves it redundantly, retracts all poses and
 * back-substitutes the depths of the frames it owns). */
int dba_ba_shard_front(const float *poses, const float *disps, const float *intrinsics, const float *disps_sens,
                       const float *targets, const float *weights, const float *eta, int eta_rows, const int64_t *ii,
                       const int64_t *jj, const uint8_t *frame_owned, int N, int B, int ht, int wd, int t0, int t1,
                       float alpha, int motion_only, void *ws, size_t ws_bytes, dba_stream_t stream);
int dba_ba_shard_back(float *poses, float *disps, const int64_t *ii, const int64_t *jj, const uint8_t *frame_owned,
                      int N, int B, int ht, int wd, int t0, int t1, float lm, float ep, int update_disps,
                      const int32_t *window_fpose, int solver_hint, void *ws, size_t ws_bytes, dba_stream_t stream);
/* window_fpose (device, t1 - t0 ints, or NULL): for every pose of the window the first pose it is coupled to in the
 * COMPLETE graph (all ranks' edges: through an edge, or through a common source frame), which lets the solver take the
 * skyline of the summed system from the graph instead of measuring it (dbaf_amd/sharded.py computes it on the host;
 * a table that names a later pose than the true one gives a wrong solve, NULL is always safe).
 * solver_hint: as for dba_ba_prepared (0 = none; 1 = meta[7] read 1 after an earlier solve of this window's summed system:
 * the several-tiles-per-thread skyline variant need not be queued behind the first one). */

/* ---- the sharded BA of one rank as ONE enqueued sequence (csrc/ba_sharded_host.hip) --------------------------------------
 * RCCL called from this library, on the caller's stream.  librccl is loaded with dlopen at the first dba_comm_* call (the copy
 * the process already has -- PyTorch ships one -- else /opt/rocm/lib); DBA_ERR_UNSUPPORTED when there is none.  The unique id
 * (128 bytes, ncclUniqueId) is made by one rank and handed to the others by the caller (dbaf_amd/sharded.py broadcasts it
 * through torch.distributed once per process group); dba_comm_create is collective and binds the calling thread's device. */
typedef struct dba_comm dba_comm;
int dba_comm_unique_id(void *id128);
int dba_comm_create(const void *id128, int world, int rank, dba_comm **out);
int dba_comm_destroy(dba_comm *c);
/* RCCL's own view of the communicator: ranks it spans, this process's rank (ncclCommCount / ncclCommUserRank) */
int dba_comm_info(dba_comm *c, int *world, int *rank);
int dba_comm_allreduce_f64(dba_comm *c, double *buf, size_t count, dba_stream_t stream);   /* in-place sum */

/* who carries what between the ranks in dba_ba_sharded_run.  world = 1: nothing is exchanged (the other fields are ignored).
 *   the reduced system [H | b] (float64, once per iteration): `comm` (RCCL all-reduce) or `peer_regions` (one-shot peer-read
 *     kernel, dba_peer_allreduce_f64: regions of all ranks, *peer_epoch is advanced by the call, peer_status as there);
 *     band_len > 0: only the entries band_idx[0..band_len) of the range travel (the skyline band of large windows, gathered
 *     into band_buf and scattered back);
 *   the inverse depths (float32, once per call, `comm` only -- a caller on the peer-read exchange gathers them itself):
 *     my_rows[n_mine] = the frames this rank owns, kmax = the largest n_mine over the ranks, send [kmax, ht*wd] /
 *     recv [world*kmax, ht*wd] staging, and for every owned row of every rank its frame all_rows[i] and its place
 *     all_slots[i] in recv. */
typedef struct {
  int world, rank;
  dba_comm *comm;
  void *const *peer_regions;
  unsigned *peer_epoch;
  size_t peer_max_doubles;
  int *peer_status;
  const int64_t *band_idx;
  size_t band_len;
  double *band_buf;
  const int64_t *my_rows;
  int n_mine, kmax;
  const int64_t *all_rows, *all_slots;
  int n_all;
  float *send, *recv;
} dba_shard_exchange;

/* stage 0 (prepared = 0 | 1 | 2 as in dba_ba_run), then dba_ba's own Gauss-Newton loop on the rank's edges -- `iterations` x
 * { linearisation (which carries the previous iteration's back-substitution + retraction, as in dba_ba: a rank moves the
 * depths of the frames it owns, the poses' update is redundant on every rank), Schur reduction, sum of [H | b] over the
 * ranks, solve with the complete graph's skyline }, the last update --, then the all-gather of the owned depth maps:
 * everything enqueued on `stream`, nothing waits on the host.  The same states as the staged sequence
 * dba_ba_shard_front / sum / dba_ba_shard_back, bit for bit.  With world = 1 nothing is summed.  The alignment gap between H
 * and b in the workspace must be zero (it is summed along). */
int dba_ba_sharded_run(float *poses, float *disps, const float *intrinsics, const float *disps_sens, const float *targets,
                       const float *weights, const float *eta, int eta_rows, const int64_t *ii, const int64_t *jj,
                       const uint8_t *frame_owned, int N, int B, int ht, int wd, int t0, int t1, int iterations, float lm,
                       float ep, float alpha, int motion_only, const int32_t *window_fpose, int solver_hint, int prepared,
                       const dba_shard_exchange *x, void *ws, size_t ws_bytes, dba_stream_t stream);

/* droid_backends.ba: `iterations` x (stage 1..4), all enqueued on `stream` with no host sync.
 * dx_out [P,6] and dz_out [>=|kx|, ht*wd] receive the last iteration's update (either may be NULL). */
int dba_ba(float *poses, float *disps, const float *intrinsics, const float *disps_sens,
           const float *targets, const float *weights, const float *eta, int eta_rows,
           const int64_t *ii, const int64_t *jj, int N, int B, int ht, int wd, int t0, int t1,
           int iterations, float lm, float ep, int motion_only, float *dx_out, float *dz_out,
           void *ws, size_t ws_bytes, dba_stream_t stream);

/* The same with stage 0 skipped: the index tables in `ws` must be those of THIS graph already, i.e. the last dba_ba /
 * dba_ba_prepare on this workspace had the same ii, jj (contents), N, B, ht, wd, t0, t1 and Schur kernel form.  For callers
 * that run several updates on one covisibility graph (CovisibleGraph.update does, dbaf/covisible_graph.py:214-342: the
 * adapter keeps one workspace per window shape and recognises an unchanged edge list, droid_backends/__init__.py).
 * Back-substitution + retraction of every iteration but the last are folded into the next iteration's linearisation in
 * both (iterations launches fewer; DBA_BA_FUSE_UPDATE=0 keeps them apart). */
int dba_ba_prepared(float *poses, float *disps, const float *intrinsics, const float *disps_sens,
                    const float *targets, const float *weights, const float *eta, int eta_rows,
                    const int64_t *ii, const int64_t *jj, int N, int B, int ht, int wd, int t0, int t1,
                    int iterations, float lm, float ep, int motion_only, float *dx_out, float *dz_out,
                    void *ws, size_t ws_bytes, dba_stream_t stream, int solver_hint);
/* solver_hint: 0 = none; 1 = meta[7] (int32 at layout.meta + 28) read 1 after an earlier call on this graph, i.e. the
 * one-tile skyline solver took its structure: the fall-back kernels behind it are then not queued (windows of 30-64
 * poses; whether it fits depends on the graph alone, a failing pivot is not a reason to fall back.  The only other thing
 * the queue was a net for, a partner workgroup more than a second late at the hand-shake, then gives a failed solve, i.e. a
 * zero update, instead of a slower correct one). */

/* dba_ba (prepared = 0) / dba_ba_prepared (prepared = 1) / stage 0 decided on the device by the graph key (prepared = 2, see
 * dba_ba_prepare_keyed; solver_hint is ignored) with the caller's next statement taken along: DepthVideo.ba clamps the inverse
 * depths right after droid_backends.ba returns (`self.disps.clamp_(min=0.001)`, dbaf/depth_video.py:560), a launch of its
 * own over the whole buffer.  disp_floor > 0: the LAST launch of the call writes max(d, disp_floor) (torch.clamp's select: a
 * NaN stays a NaN) for the frames it updates and applies the same floor to every other frame of the buffer (also when
 * motion_only leaves the depths alone): the same state, bit for bit, as the call followed by the caller's clamp over the
 * whole buffer -- the reference's caller rescales inverse depths between BA calls (dbaf_frontend.py:570,814), so frames
 * outside kx can be below the floor as well.  Earlier iterations and the
 * returned dz are untouched, exactly as when the clamp follows the call.  disp_floor = 0: dba_ba / dba_ba_prepared. */
int dba_ba_run(float *poses, float *disps, const float *intrinsics, const float *disps_sens,
               const float *targets, const float *weights, const float *eta, int eta_rows,
               const int64_t *ii, const int64_t *jj, int N, int B, int ht, int wd, int t0, int t1,
               int iterations, float lm, float ep, int motion_only, float *dx_out, float *dz_out,
               void *ws, size_t ws_bytes, dba_stream_t stream, int prepared, int solver_hint, float disp_floor);

/* dba_bacore_hessian with stage 0 as in dba_ba_run (prepared = 0 | 1 | 2): BACore.hessian runs twice per update on one
 * graph (dbaf/depth_video.py:527), the second call finds the tables in place */
int dba_bacore_hessian_run(const float *poses, const float *disps, const float *intrinsics,
                           const float *disps_sens, const float *targets, const float *weights,
                           const float *eta, int eta_rows, const int64_t *ii, const int64_t *jj, int N,
                           int B, int ht, int wd, int t0, int t1, double *H_host, double *v_host,
                           void *ws, size_t ws_bytes, dba_stream_t stream, int prepared);

/* BACore::hessian with the reduced system handed over in PINNED HOST MEMORY OF THE LIBRARY (one block per workspace, valid until
 * the next hessian call on that workspace): *out_host.  The last kernel of the sequence writes the system there itself -- mirrored
 * from the lower triangle the reduction keeps up -- and sets a completion word the call spins on: no copy engine, no stream
 * synchronisation (round 5: two hipMemcpyAsync + hipStreamSynchronize, 94 us per call on the 25-KF window).
 * layout 0: H [6P, 6P] row-major followed by v [6P] (what src/droid_kernels.cu:1889-1897 copies out).
 * layout 1: the system in the factor-graph side's tangent coordinates, as the augmented matrix [Hg | vg] of shape [6P, 6P + 1]
 *   that the GTSAM fork's BA2GTSAM returns (/root/reference/dbaf/depth_video.py:20-29, :397-401, :527-529):
 *   Hg = J^T (H + stabilizer on the first pose's diagonal, :397) J, vg = J^T v, J = blockdiag(A36), A36 the row-major 6 x 6 block
 *   -Ad(Tbc^-1) with its row halves swapped (:21-23).  A36 is ignored for layout 0. */
int dba_bacore_hessian_host(const float *poses, const float *disps, const float *intrinsics,
                            const float *disps_sens, const float *targets, const float *weights,
                            const float *eta, int eta_rows, const int64_t *ii, const int64_t *jj, int N,
                            int B, int ht, int wd, int t0, int t1, void *ws, size_t ws_bytes, dba_stream_t stream,
                            int prepared, int layout, const double *A36, double stabilizer, double **out_host);

/* where this workspace's pinned block is (what the last hessian / export call on it filled); error if there is none yet */
int dba_bacore_staging(int N, int B, int ht, int wd, int t0, int t1, void *ws, size_t ws_bytes, double **out_host);

/* the last step of dba_bacore_hessian_host alone: the reduced system that lies in the workspace (H lower triangle, b: after
 * dba_ba_reduce, or after a sum over ranks) -> the workspace's pinned block, layout as above; waits for completion. */
int dba_bacore_export_host(int N, int B, int ht, int wd, int t0, int t1, void *ws, size_t ws_bytes, dba_stream_t stream, int layout,
                           const double *A36, double stabilizer, double **out_host);

/* BACore::hessian: stages 1-2 with alpha = 0.001, then copies H [6P,6P], v [6P] (float64) to HOST
 * memory (the caller owns CPU tensors, src/droid_kernels.cu:1889-1897): dba_bacore_hessian_host + two host memcpys; complete
 * on return. */
int dba_bacore_hessian(const float *poses, const float *disps, const float *intrinsics,
                       const float *disps_sens, const float *targets, const float *weights,
                       const float *eta, int eta_rows, const int64_t *ii, const int64_t *jj, int N,
                       int B, int ht, int wd, int t0, int t1, double *H_host, double *v_host, void *ws,
                       size_t ws_bytes, dba_stream_t stream);

/* BACore::retract: dx_host [6P] float64 (HOST) -> f32 on device, then stage 4 using the E, Q, w
 * cached by the last dba_bacore_hessian on the same workspace.  Up to 64 poses the update travels as a kernel argument:
 * dx_host is consumed before the call returns and nothing synchronises the stream. */
int dba_bacore_retract(float *poses, float *disps, const int64_t *ii, const int64_t *jj, int N, int B,
                       int ht, int wd, int t0, int t1, const double *dx_host, float *dx_out,
                       float *dz_out, void *ws, size_t ws_bytes, dba_stream_t stream);

/* BACore::optimize: damped dense solve of a caller-supplied HOST system (solveDenseD :200-218);
 * result kept in the workspace dx slot and copied to dx_out (device, may be NULL). */
int dba_bacore_optimize(const double *H_host, const double *v_host, int N, int B, int ht, int wd,
                        int t0, int t1, float lm, float ep, float *dx_out, void *ws, size_t ws_bytes,
                        dba_stream_t stream);

/* Marginal variances of the inverse depths of the window, from the system the last linearisation + reduction on `ws` left
 * there (csrc/depth_variance.hip).  With E [(P+N), 6, HW] (rows 0..P-1: a frame's own pose; row P + n: edge n, pose jj[n],
 * depths of frame ii[n]), Q = 1 / C [|kx|, HW] (float32) and the LOWER triangle of H = A - E Q E^T (float64):
 *     Sd = H + diag(ep + lm diag(H))      -- what dba_ba_solve factorises --,   M = Sd^-1,
 *     var_out[f, k] = Q[m, k] + Q[m, k]^2 * sum over r, s in rows(f) of  E[r, :, k]^T M[pose(r) block, pose(s) block] E[s, :, k]
 * for every slot m of kx (f = kx[m]) and pixel k; rows(f) = the rows of E whose depths are frame f's and whose pose lies
 * inside [t0, t1).  This is the k-th diagonal entry of the depth block of the inverse of [[Sd + E Q E^T, E], [E^T, C]]: the
 * covariance of the inverse depths given the poses before t0, under the damping of the step.  A frame without such a row gets Q.
 * All sums in float64, no atomics (bit-identical from run to run), three launches on `stream`, no host synchronisation.
 *   var_out [out_rows, ht, wd] float32, addressed by frame id like disps; rows of frames outside kx are not written.
 *   scratch: device memory of dba_ba_depth_variance_scratch_bytes(t1 - t0) bytes (0: P unsupported), aligned to 8; it holds
 *     the factor, M and a status word -- the workspace does not grow.  Reads the tables of stage 0 (kx, eoff, einfo): no ii, jj.
 *   A pivot of the factorisation that is not positive is no error code: every written row is NaN (the reference's solve
 *     degrades silently too).  H, E, Q, dx and meta are not modified; the solvers do not modify H either, so the call is valid
 *     from the reduction until the next linearisation on `ws`, before or after dba_ba_solve / dba_ba_update / dba_bacore_retract.
 * Returned BEFORE ANY RUNTIME CALL: DBA_ERR_ARG for a null or misaligned pointer, sizes ba_plan refuses, P < 1 or
 * out_rows < B; DBA_ERR_UNSUPPORTED for P > 64 or N > 1023; DBA_ERR_WORKSPACE for a workspace or scratch that is too small. */
size_t dba_ba_depth_variance_scratch_bytes(int P);
int dba_ba_depth_variance(int N, int B, int ht, int wd, int t0, int t1, float lm, float ep, float *var_out, int out_rows,
                          void *scratch, size_t scratch_bytes, void *ws, size_t ws_bytes, dba_stream_t stream);
/* the same, one part at a time (tools/bench_depth_variance.py): parts = 1: M = Sd^-1 into the scratch (two launches), 2: the
 * quadratic form with the M an earlier call left in THIS scratch (one launch), 3: both; anything else is DBA_ERR_ARG */
int dba_ba_depth_variance_parts(int N, int B, int ht, int wd, int t0, int t1, float lm, float ep, float *var_out, int out_rows,
                                void *scratch, size_t scratch_bytes, void *ws, size_t ws_bytes, dba_stream_t stream, int parts);

/* 6 x 6 covariances of the window's poses, from the system the last linearisation + reduction on `ws` left there
 * (csrc/pose_covariance.hip; the factor and the column solve are those of dba_ba_depth_variance, csrc/reduced_inverse.h).  With
 *     Sd = H + diag(ep + lm diag(H)),   M = Sd^-1   (H: the LOWER triangle, float64)
 * the blocks of M are the covariances of the pose tangents given the gauge -- the poses outside [t0, t1), which BA keeps fixed --
 * with the depths marginalised out, under the damping of the step.  Tangents are this library's: (tau, phi), applied on the left
 * of the world -> camera pose, T' = Exp(xi) T.
 *   marginal job k:  out_marg[k] = S_bb = M[6p:6p+6, 6p:6p+6], p = marg[k] - t0.  With Ainv (6 x 6 row-major, HOST, may be NULL)
 *       out_marg[k] = Ainv S_bb Ainv^T: with Ainv = A^-1, A the block of dba_bacore_hessian_host's layout 1 (dx_ba = A dx_g), the
 *       covariance in the factor-graph side's tangent coordinates.  Ainv applies to marginal jobs ONLY.
 *   relative job k = (a, b) = (pairs[2k], pairs[2k+1]):  with G = T_b T_a^-1 = (R, t) and Ad = Ad(G) = [[R, [t]x R], [0, R]],
 *       out_pairs[k] = S_bb + Ad S_aa Ad^T - Ad S_ab - S_ba Ad^T,
 *       the first-order covariance of xi_rel in G' = Exp(xi_rel) G, xi_rel = xi_b - Ad xi_a: ALWAYS in camera tangents.  A frame
 *       outside [t0, t1) is a fixed pose, its blocks of S are zero: (a < t0, b) gives S_bb.  Ad is formed in float64 from
 *       `poses` [B, 7] (t, q_xyzw; q normalised in float64) as stored when the kernel runs.
 *   marg [n_marg], pairs [2 n_pairs]: HOST arrays of frame indices; they and Ainv are consumed before the call returns (they
 *   travel in the kernel's argument block: no copy, no host synchronisation, the call records into a hipGraph).
 *   out_marg [out_marg_rows >= n_marg, 6, 6], out_pairs [out_pair_rows >= n_pairs, 6, 6]: float64, device; rows beyond the job
 *   count are not written.  Every block is written from its lower triangle and mirrored: symmetric to the bit.  Without Ainv a
 *   marginal block holds the bits dba_ba_depth_variance_parts(parts = 1) leaves in the lower triangle of that block of M.
 *   scratch: as for dba_ba_depth_variance (the same size, the same layout; the M part is not touched).
 * All arithmetic in float64, no atomics (bit-identical from run to run), two launches on `stream`: the factor, then one
 * workgroup per job.  A pivot that is not positive is no error code: every block is NaN.  Nothing in the workspace is modified
 * (meta[1] included); valid from the reduction until the next linearisation on `ws`, before or after a solve or a retraction.
 * Returned BEFORE ANY RUNTIME CALL: DBA_ERR_ARG for a null or misaligned pointer (poses, pairs, out_pairs only with n_pairs > 0;
 * marg, out_marg only with n_marg > 0), no job at all, more than 64 marginal jobs or 64 pairs, an output with fewer rows than
 * jobs, a frame index outside [0, B), a marginal index outside [t0, t1), a pair with a == b, sizes ba_plan refuses, P < 1;
 * DBA_ERR_UNSUPPORTED for P > 64; DBA_ERR_WORKSPACE for a workspace or scratch that is too small. */
int dba_ba_pose_covariance(const float *poses, int N, int B, int ht, int wd, int t0, int t1, float lm, float ep, const int *marg,
                           int n_marg, const int *pairs, int n_pairs, const double *Ainv, double *out_marg, int out_marg_rows,
                           double *out_pairs, int out_pair_rows, void *scratch, size_t scratch_bytes, void *ws, size_t ws_bytes,
                           dba_stream_t stream);

/* dba_bacore_retract with the increment in DEVICE memory: dx_dev [6 (t1 - t0)] float64, BA tangents, is rounded to float32 into
 * the workspace's update slot and applied by the same back-substitution + retraction launch.  skip_dev (device, may be NULL):
 * when the word it points to is not zero as the launches run, neither poses nor inverse depths move and dx_out, dz_out are not
 * written.  No host synchronisation; two launches.  DBA_ERR_ARG for a null dx_dev, poses, disps or jj and for sizes ba_plan
 * refuses, DBA_ERR_WORKSPACE for a workspace that is too small: before any runtime call. */
int dba_bacore_retract_device(float *poses, float *disps, const int64_t *ii, const int64_t *jj, int N, int B, int ht, int wd, int t0,
                              int t1, const double *dx_dev, const int *skip_dev, float *dx_out, float *dz_out, void *ws,
                              size_t ws_bytes, dba_stream_t stream);

/* Inertial factors in the window solve (csrc/inertial.hip; dbaf_amd/inertial.py is the public interface and states the
 * residual).  P inertial states, world <- body, all float64 on the device: R [P, 3, 3] row-major, p [P, 3], vel [P, 3],
 * bias [P, 6] = (ba, bg).  The tangent of a state is (dphi, dp, dv, dba, dbg): R <- R Exp(dphi), p <- p + R dp, vel += dv,
 * bias += db; (dphi, dp) are the coordinates dba_bacore_hessian_host's layout 1 delivers the visual system in.
 * Optional diagonal priors: anchors prior_R, prior_p, prior_vel, prior_bias (shaped like the state) and prior_w [P, 15] =
 * mask / sigma^2 per tangent entry; all five NULL: no prior.  The residual of a prior is the tangent at the anchor that
 * leads to the state.
 * preint [preint_rows >= P - 1, DBA_INERTIAL_K]: one row per interval k -> k + 1,
 *     dR 9 | dv 3 | dp 3 | dt 1 | dR/dbg 9 | dv/dba 9 | dv/dbg 9 | dp/dba 9 | dp/dbg 9 | linearisation bias 6 | L9 81 | L6 36
 * (matrices row-major; L9 the INVERSE of the 9 x 9 covariance in the order phi, v, p; L6 the inverse of the bias random walk's).
 * The struct is read on the host (pointers and gravity travel as kernel arguments); what it points to is device memory. */
#define DBA_INERTIAL_K 184
#define DBA_INERTIAL_MAX_P 25 /* 15 P <= 384: the one-workgroup float64 Cholesky of csrc/reduced_inverse.h */
typedef struct {
  double *R, *p, *vel, *bias;
  const double *prior_R, *prior_p, *prior_vel, *prior_bias, *prior_w;
  double gravity[3];
  /* The dense prior over the first dense_K states (1 <= dense_K <= P), float64 on the device; all six NULL and dense_K = 0:
   * none.  Linearisation point dense_R [K, 3, 3], dense_p [K, 3], dense_vel [K, 3], dense_bias [K, 6]; dense_H [15 K, 15 K]
   * (symmetric), dense_b [15 K].  Its energy is delta^T H delta / 2 - b^T delta with, per state,
   *     delta = (Log(R0^T R), R0^T (p - p0), vel - vel0, bias - bias0);
   * it adds H to the first 15 K rows and columns of the step's system and b - H delta to its right-hand side (the Jacobian of
   * delta is not applied: the relinearisation of a linear container factor). */
  const double *dense_R, *dense_p, *dense_vel, *dense_bias, *dense_H, *dense_b;
  int dense_K;
} dba_inertial_state;

/* bytes of the scratch both entries below work in for P states; 0 for a P they refuse */
size_t dba_inertial_scratch_bytes(int P);

/* Launch (a) alone: per interval r [15], J^T L J [30, 30] and J^T L r [30] over the tangents of its two states, and per state
 * the prior's terms (into the scratch).  r_out [>= P - 1, 15], H_out [>= P - 1, 30, 30], g_out [>= P - 1, 30]: float64,
 * device, each may be NULL (the scratch's own slots are always written).  One launch, one workgroup per state, no atomics.
 * Refused BEFORE ANY RUNTIME CALL: DBA_ERR_ARG for a null st, R, p, vel, bias, preint or scratch, priors given in part,
 * a misaligned pointer, P < 2 or preint_rows < P - 1; DBA_ERR_UNSUPPORTED for P > DBA_INERTIAL_MAX_P; DBA_ERR_WORKSPACE for
 * scratch_bytes < dba_inertial_scratch_bytes(P). */
int dba_inertial_linearize(const dba_inertial_state *st, int P, const double *preint, int preint_rows, double *r_out,
                           double *H_out, double *g_out, void *scratch, size_t scratch_bytes, dba_stream_t stream);

/* One visual-inertial Gauss-Newton step on the device, after a linearisation + reduction (dba_bacore_hessian_host) on `ws`:
 *   (a) dba_inertial_linearize;
 *   (b) the 15 P x 15 P system M dx = rhs in one fixed order, every entry owned by one lane, no atomics: the window's H, v read
 *       from the workspace, with `stabilizer` on the first six diagonal entries and the congruence by A36 (6 x 6 row-major,
 *       HOST: the block of dba_bacore_hessian_host's layout 1, dx_ba = A dx_g) exactly as that entry's export applies them,
 *       in the pose slots; then the interval before the state, the interval after it, the prior.  rhs = vg - sum J^T L r;
 *   (c) Md = M + diag(ep + lm diag(M)) = L L^T and the two substitutions, by the kernels of csrc/reduced_inverse.h;
 *   (d) the retraction of the inertial states, dx_ba = A dx_g for the pose part, and dba_bacore_retract_device.
 * dx_out [P, 15] float64, device.  status_out (device int, may be NULL): 1 when a pivot was not positive -- then dx_out is NaN
 * and neither the inertial states nor poses nor inverse depths move -- else 0.  Six launches, all float64, bit-identical from
 * run to run, no host synchronisation (records into a hipGraph).  poses, disps, ii, jj, N .. t1, ws as for dba_bacore_retract.
 * Refused BEFORE ANY RUNTIME CALL: what dba_inertial_linearize refuses, a null A36, dx_out, poses, disps or jj, sizes ba_plan
 * refuses or a window that is not P poses wide (DBA_ERR_ARG), a workspace that is too small (DBA_ERR_WORKSPACE). */
int dba_inertial_step(const dba_inertial_state *st, int P, const double *preint, int preint_rows, const double *A36,
                      double stabilizer, float lm, float ep, float *poses, float *disps, const int64_t *ii, const int64_t *jj, int N,
                      int B, int ht, int wd, int t0, int t1, double *dx_out, int *status_out, void *scratch, size_t scratch_bytes,
                      void *ws, size_t ws_bytes, dba_stream_t stream);

/* bytes of the scratch dba_inertial_marginalize works in for a window of P states (what dba_inertial_scratch_bytes(P) returns:
 * one scratch serves both entries); 0 for a P they refuse */
size_t dba_inertial_marg_scratch_bytes(int P);

/* Marginalise the m oldest of the P states into a dense prior over the states that stay coupled to them (the reference's
 * gtsam.marginalizeOut, dbaf/depth_video.py:357-443), at the current states, on the device.  The system over
 * S = max(Pm, m + 1, dense_K) states takes, per entry and in this order: the reduced camera system of the MARGINAL BA window in
 * `ws` (Pm = t1 - t0 poses, its pose 0 is state 0; `stabilizer` and A36 as dba_inertial_step applies them; ws NULL: Pm = 0 and
 * N .. t1 are not read), the intervals k -> k + 1 for k < m, the diagonal priors of the states < m, and the whole dense prior
 * of `st`, relinearised.  No damping.  With mm = the first 15 m unknowns and kk = the other 15 (S - m):
 *     H_new = M_kk - M_km M_mm^-1 M_mk,   b_new = rhs_k - M_km M_mm^-1 rhs_m,
 * the linearisation point = the states m .. S - 1.  K_new = S - m.
 *   H_new [h_rows >= 15 K_new rows of its own length]: written dense, [15 K_new, 15 K_new] row-major, symmetric to the bit;
 *   b_new [b_rows >= 15 K_new]; R0 [x0_rows, 3, 3], p0 [x0_rows, 3], vel0 [x0_rows, 3], bias0 [x0_rows, 6], x0_rows >= K_new.
 *   None of them may be memory of the dense prior in `st`, which is only read.
 *   status_out (device int, may be NULL): 1 when M_mm had a pivot that was not positive -- then H_new and b_new are NaN and
 *   nothing else is written -- else 0.
 * Five launches (the linearisation, the assembly in three dense parts, the factor of M_mm, one forward substitution per column
 * over as many workgroups, the Schur products), all float64, no atomics, no host synchronisation, bit-identical from run to run.
 * Refused BEFORE ANY RUNTIME CALL: what dba_inertial_linearize refuses (a dense prior given in part or with dense_K outside
 * [1, P] among it), a null or misaligned A36 or output, m < 1, m >= P, Pm > P, a capacity below K_new, sizes ba_plan refuses
 * (DBA_ERR_ARG); P > DBA_INERTIAL_MAX_P (DBA_ERR_UNSUPPORTED); a short scratch or BA workspace (DBA_ERR_WORKSPACE). */
int dba_inertial_marginalize(const dba_inertial_state *st, int P, const double *preint, int preint_rows, const double *A36,
                             double stabilizer, int m, int N, int B, int ht, int wd, int t0, int t1, void *ws, size_t ws_bytes,
                             double *H_new, int h_rows, double *b_new, int b_rows, double *R0, double *p0, double *vel0,
                             double *bias0, int x0_rows, int *status_out, void *scratch, size_t scratch_bytes, dba_stream_t stream);

/* The BA cost report (csrc/ba_cost.hip): what the linearisation minimises, per edge.  For edge n with i = ii[n], j = jj[n] and
 * pixel k = v * wd + u: Gij = Tj Ti^-1 (i == j: the fixed stereo baseline t = (-0.1, 0, 0), q = identity) formed in float64
 * and rounded once, X = ((u - cx) / fx, (v - cy) / fy, 1), d = disps[i, k], (x, y, z) = R X + d t.  A pixel with z < 0.25 is
 * cut.  Otherwise r_u = targets[n, 0, k] - (fx x / z + cx), r_v = targets[n, 1, k] - (fy y / z + cy), w_u = 0.001 weights[n, 0, k],
 * w_v = 0.001 weights[n, 1, k] -- the float32 expressions of ba_linearize_kernel; a stereo edge keeps its weights (the residual
 * its depth block sees).  A pixel is used if it is not cut and w_u + w_v != 0.  Over the used pixels of the edge, in float64:
 *     out[n] = (cost = sum w_u r_u^2 + w_v r_v^2,  wsum = sum w_u + w_v,  n_used = their number,  r2max = max r_u^2 + r_v^2),
 * (0, 0, 0, 0) without a used pixel; out[N] = the sums of cost, wsum, n_used and the max of r2max over the rows as stored.
 *   out [out_rows >= N + 1, 4] float64 on the device; rows beyond N are not written.
 *   scratch: dba_ba_cost_scratch_bytes(N, ht, wd) = 32 N ceil(ht wd / 1024) bytes of device memory, aligned to 16 (0 for N == 0
 *     and for sizes the call refuses); four doubles per (edge, slice of 1024 pixels).  No BA workspace is needed or touched.
 *   A NaN among a used pixel's inputs makes that edge's cost and r2max NaN, and the total's; no other row changes.  An edge
 *   whose ii or jj lies outside [0, B) reads (NaN, NaN, -1, NaN) and nothing is read through the index.
 * Two launches on `stream` (N == 0: one, which writes a zero total row), no atomics -- the same bytes from run to run and from
 * device to device --, no host synchronisation.  Returned BEFORE ANY RUNTIME CALL: DBA_ERR_ARG for a null or misaligned pointer
 * (N == 0 needs `out` alone), N < 0, B < 1, ht or wd < 1, out_rows < N + 1; DBA_ERR_UNSUPPORTED when N ceil(ht wd / 1024) or
 * ht wd exceeds 2^31 - 1; DBA_ERR_WORKSPACE for a scratch that is too small. */
size_t dba_ba_cost_scratch_bytes(int N, int ht, int wd);
int dba_ba_cost(const float *poses, const float *disps, const float *intrinsics4, const float *targets, const float *weights,
                const int64_t *ii, const int64_t *jj, int N, int B, int ht, int wd, double *out, int out_rows, void *scratch,
                size_t scratch_bytes, dba_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Correlation volume: CorrBlock (dbaf/modules/corr.py:24-71) and its lookup
 * droid_backends.corr_index_forward (src/droid.cpp:231-239, src/correlation_kernels.cu:19-70,126-155).
 * ---------------------------------------------------------------------------------------- */

/* corr_index_forward: volume [n,h1,w1,h2,w2] (dtype), coords [n,2,h1,w1] f32 (ch0 = x, ch1 = y)
 * -> corr [n,2r+1,2r+1,h1,w1] (dtype), channel = x_offset*(2r+1) + y_offset.  Bit-exact with the
 * reference arithmetic (four c10::Half read-modify-writes per tap in a fixed order). */
int dba_corr_index_forward(const void *volume, const float *coords, void *corr, int n, int h1, int w1,
                           int h2, int w2, int radius, int dtype, dba_stream_t stream);

/* fused CorrBlock.__call__ (corr.py:40-50): all pyramid levels in one launch, reading
 * coords [n,h1,w1,2] as produced by projective_transform and writing the concatenated
 * [n, L*(2r+1)^2, h1, w1] tensor directly (no per-level tensors, no torch.cat).
 * level l volume: [n,h1,w1,h2>>l,w2>>l]; coords are divided by 2^l per level. */
int dba_corr_lookup_pyramid(const void *const *volumes /* host array of L device ptrs */,
                            const float *coords_nhw2, void *corr, int n, int h1, int w1, int h2,
                            int w2, int num_levels, int radius, int dtype, dba_stream_t stream);

/* Flow-aligned ("sheared") volume: Vs_l[n][dy][dx][pixel] = V_l[n][y1][x1][ty][tx] with pixel = y1 * w1 + x1,
 * dy = (ty - (y1 >> l)) mod h2l, dx = (tx - (x1 >> l)) mod w2l; the pixel axis is padded to
 * dba_corr_sheared_plane_elems(h1, w1) = h1 * w1 rounded up to a multiple of 64, or the size of the tile grid for tiled planes
 * (dba_corr_sheared_grid; padding is never read for a real pixel) -- the size of the reference tensor of dbaf/modules/corr.py:31-36 (+ padding), but the taps that
 * neighbouring source pixels read become contiguous, so a wave fetches full, aligned 128-byte lines for ANY map
 * size (csrc/corr_sheared.hip).  Used by the CorrBlock mirror; the lookup result is bit-identical to
 * corr_index_forward on the reference layout.  f16 only, radius 3. */
int dba_corr_sheared_plane_elems(int h1, int w1);
/* Order of the pixel axis.  Maps with h1 % 4 == 0 and w1 % 16 == 0 keep their source pixels in 4 x 16 TILES,
 * pixel = ((y1 >> 2) * (w1 >> 4) + (x1 >> 4)) * 64 + (y1 & 3) * 16 + (x1 & 15), so that the 64 pixels of a 128-byte line are
 * neighbours in BOTH directions: the union of their windows -- what a lookup wave reads -- is 79 instead of 92 lines per wave
 * and level on the bench scene, and the lookup's time is proportional to that number (profiles/r04_lookup_lines.txt).  Other
 * maps: pixel = y1 * w1 + x1.  Returns the tile width (16) for the tiled order, 0 for the row-major one (DBA_SHEAR_TILES=0
 * keeps every shape row-major). */
int dba_corr_sheared_tiled(int h1, int w1);
/* ... and the grid the tiles are counted on: (h1g, w1g) = (h1, w1) rounded up to multiples of (4, 64) for tiled planes (then
 * dba_corr_sheared_plane_elems = h1g * w1g; the pad pixels' entries are never read as taps), (h1, w1) itself for linear ones.
 * Returns the tile width like dba_corr_sheared_tiled.  With DBA_SHEAR_PAD=1 (opt-in, read once per process) maps within 25 % of
 * such a grid are tiled on it (28 x 107 on 28 x 128, 55 x 55 on 56 x 64); coordinates and the returned tensors keep the map's own
 * [h1, w1] indexing.  By default only the maps that ARE such a grid are tiled. */
int dba_corr_sheared_grid(int h1, int w1, int *h1g, int *w1g);
/* which form of the sheared lookup dba_corr_lookup_pyramid_sheared launches: 0 = automatic (by map shape), 2 = resident
 * (any shape), 5 = rows over tiles (tiled planes only, falls back to resident otherwise).  Process-wide; results are
 * bit-identical.  (1, 3, 4 were round 4's streaming / pair / band forms, which no longer ship: DBA_ERR_ARG.) */
int dba_corr_lookup_select(int kernel);
/* Measurement hook: the next dba_corr_lookup_pyramid_sheared call of this thread attaches the two hipEvent_t to its
 * kernel dispatch (hipExtLaunchKernelGGL: the dispatch's own start / end timestamps, no marker packets in the stream),
 * then disarms.  hipEventElapsedTime(start, stop) is the kernel's duration; bench.py times the roofline kernel this
 * way in every timed step.  NULL, NULL disarms. */
int dba_corr_lookup_arm_timing(void *start_event, void *stop_event);
/* Fused build of the sheared pyramid straight from the feature maps (csrc/corr_build_fused.hip): MFMA GEMM,
 * 2x2 pooling of the rounded levels and the flow-aligned store in one pass; every output byte is written once.
 * Supported when dba_corr_volume_build_sheared_supported(...) returns 1 (w2 <= 128, C % 16 == 0, 4 levels, every
 * level non-empty); sheared_levels[l] is [n, h2>>l, w2>>l, dba_corr_sheared_plane_elems(h1, w1)] f16.  scratch as for
 * dba_corr_volume_build.  Source and target maps may differ in size as long as every source row and column is a residue
 * of the target map after ONE conditional wrap (h1 <= h2 + 1 and w1 <= w2 + 1: the kernels' dy and dx take a single
 * correction); larger source maps are not supported. */
int dba_corr_volume_build_sheared_supported(int C, int h1, int w1, int h2, int w2, int num_levels);
/* Which kernel dba_corr_volume_build_sheared[_slots] launches for a shape: a pure host decision (the shape, the planes' pixel
 * order and the DBA_BUILD_KERNEL / DBA_BUILD_OPERANDS / DBA_BUILD_WAVES switches, each read once per
 * process); nothing is launched.  The launcher switches on the same value. */
enum dba_corr_build_route {
  DBA_CORR_ROUTE_UNFUSED = 0,       /* not supported: dba_corr_volume_build + dba_corr_shear_level */
  DBA_CORR_ROUTE_FUSED16 = 1,       /* corr_build_fused16_kernel: sixteen waves, tiled planes, 64 columns, the maps as they lie */
  DBA_CORR_ROUTE_FUSED16G = 2,      /* corr_build_fused16g_kernel<0>: sixteen waves, linear planes, 33..63 unaligned columns */
  DBA_CORR_ROUTE_FUSED16G_55 = 3,   /* corr_build_fused16g_kernel<55> */
  DBA_CORR_ROUTE_FUSED16W = 4,      /* corr_build_fused16w_kernel: sixteen waves, linear planes, 65..128 columns */
  DBA_CORR_ROUTE_WALK_NATIVE = 5,   /* corr_build_fused_kernel<2, true, true>: strip walk, both maps as they lie */
  DBA_CORR_ROUTE_WALK_NATIVE_B = 6, /* corr_build_fused_kernel<2, true, false, true>: strip walk, the target map as it lies */
  DBA_CORR_ROUTE_WALK_COPY = 7,     /* corr_build_fused_kernel<2, true>: strip walk on the k-block-major copies */
  DBA_CORR_ROUTE_STRIP_64 = 8,      /* corr_build_fused_kernel<2, false>: one strip per workgroup, up to 64 columns */
  DBA_CORR_ROUTE_STRIP_128 = 9      /* corr_build_fused_kernel<4, false>: one strip per workgroup, 65..128 columns */
};
int dba_corr_volume_build_route(int C, int h1, int w1, int h2, int w2, int num_levels);
int dba_corr_volume_build_sheared(const void *fmap1, const void *fmap2, void *const *sheared_levels, int n, int C,
                                  int h1, int w1, int h2, int w2, int num_levels, void *scratch,
                                  size_t scratch_bytes, dba_stream_t stream);
int dba_corr_shear_level(const void *ref_level, void *sheared_level, int n, int h1, int w1, int h2l, int w2l,
                         int lvl, dba_stream_t stream);
int dba_corr_lookup_pyramid_sheared(const void *const *volumes /* host array of L device ptrs */,
                                    const float *coords_nhw2, void *corr, int n, int h1, int w1, int h2,
                                    int w2, int num_levels, int radius, dba_stream_t stream);

/* Slot-addressed pyramid (the MI355X form of CorrBlock.cat / CorrBlock.__getitem__, dbaf/modules/corr.py:52-60, which the
 * reference runs as torch.cat / boolean indexing of the WHOLE pyramid on every add_factors / rm_factors,
 * dbaf/covisible_graph.py:131,166).  A level store holds `capacity` edge volumes; edge e of a lookup lives in slot
 * slots[e] (device int32 [n]; NULL = slot e).  New edges are built straight into free slots (out_slots[e]: where edge e of
 * this build goes), removing or re-ordering edges edits the table: no volume is moved. */
int dba_corr_volume_build_sheared_slots(const void *fmap1, const void *fmap2, void *const *level_stores,
                                        const int *out_slots /* device [n] or NULL */, int n, int C, int h1, int w1, int h2,
                                        int w2, int num_levels, void *scratch, size_t scratch_bytes, dba_stream_t stream);
int dba_corr_lookup_pyramid_sheared_slots(const void *const *level_stores, const int *slots /* device [n] or NULL */,
                                          const float *coords_nhw2, void *corr, int n, int h1, int w1, int h2, int w2,
                                          int num_levels, int radius, dba_stream_t stream);
int dba_corr_lookup_pyramid_slots(const void *const *level_stores, const int *slots, const float *coords_nhw2, void *corr,
                                  int n, int h1, int w1, int h2, int w2, int num_levels, int radius, int dtype,
                                  dba_stream_t stream);

/* The lookup with the reprojection in its prologue: pops.projective_transform (dbaf/geom/projective_ops.py:96-125, via
 * DepthVideo.reproject, dbaf/depth_video.py:221-229) + CorrBlock.__call__ (dbaf/modules/corr.py:40-50) in ONE launch.
 * poses [B,7], disps [B,h1,w1], intrinsics_b4 [B,4] (per frame), ii, jj [n] int64; the coordinates are computed per pixel
 * (csrc/reproj.h: the arithmetic of dba_reproject, bit for bit) and never read back; coords_out [n,h1,w1,2] and valid_out
 * [n,h1,w1,1] (either may be NULL) receive what dba_reproject would have written -- the caller needs them for the motion
 * features and the BA targets (dbaf/covisible_graph.py:220-221,237).  corr is bit-identical to dba_reproject followed by
 * dba_corr_lookup_pyramid_sheared_slots. */
int dba_corr_lookup_reproject_sheared(const void *const *level_stores, const int *slots, const float *poses,
                                      const float *disps, const float *intrinsics_b4, const int64_t *ii, const int64_t *jj,
                                      float *coords_out, float *valid_out, void *corr, int n, int h1, int w1, int h2, int w2,
                                      int num_levels, int radius, dba_stream_t stream);

/* The same launch with the motion features of CovisibleGraph.update() riding along (dbaf/covisible_graph.py:221-222):
 *     motn = torch.cat([coords1 - coords0, target - coords1], dim=-1).permute(0,1,4,2,3).clamp(-64.0, 64.0)
 * target [n,h1,w1,2] f32 is the edges' previous target (pixel-interleaved, 8-byte aligned), motn [n,4,h1,w1] f32 (planar)
 * receives, from the lane of pyramid level 0 that writes the pixel's coords_out, clamp(cx - x1), clamp(cy - y1),
 * clamp(tx - cx), clamp(ty - cy): one float32 subtraction each, coords0 = the pixel's own (x1, y1), and a clamp that is a
 * compare-select, so a NaN passes as it does through torch.clamp.  Bit-identical to the two statements run with torch on
 * the device; corr, coords_out and valid_out are the bytes dba_corr_lookup_reproject_sheared writes.  target and motn
 * must not be NULL; the kernels are instantiations of their own, the lookups above are compiled as before. */
int dba_corr_lookup_reproject_motion_sheared(const void *const *level_stores, const int *slots, const float *poses,
                                             const float *disps, const float *intrinsics_b4, const int64_t *ii,
                                             const int64_t *jj, float *coords_out, float *valid_out, void *corr,
                                             const float *target, float *motn, int n, int h1, int w1, int h2, int w2,
                                             int num_levels, int radius, dba_stream_t stream);

/* A pyramid that is built, looked up ONCE and dropped -- MotionFilter.track, dbaf/motion_filter.py:74-76:
 * `corr = CorrBlock(self.fmap[None,[0]], gmap[None,[0]])(coords0)`, once per incoming frame -- as one call: the levels go into
 * `pyramid` (device scratch of dba_corr_once_pyramid_bytes bytes that the caller keeps per stream and reuses from frame to frame:
 * calls on one stream are ordered), then the fused lookup reads them.  = dba_corr_volume_build_sheared_slots followed by
 * dba_corr_lookup_pyramid_sheared_slots with identity slots, bit for bit; what it saves is the host's share (four level
 * allocations and one library call per frame).  DBA_ERR_UNSUPPORTED where dba_corr_volume_build_sheared_supported says no. */
size_t dba_corr_once_pyramid_bytes(int n, int h1, int w1, int h2, int w2, int num_levels);
int dba_corr_build_lookup_once_sheared(const void *fmap1, const void *fmap2, const float *coords_nhw2, void *corr, void *pyramid,
                                       size_t pyramid_bytes, void *scratch, size_t scratch_bytes, int n, int C, int h1, int w1,
                                       int h2, int w2, int num_levels, int radius, dba_stream_t stream);

/* ONE level of the flow-aligned pyramid looked up with the arguments droid_backends.corr_index_forward receives from the
 * reference's unmodified CorrBlock.__call__ (dbaf/modules/corr.py:40-50): coords [n, 2, h1, w1] ALREADY divided by 2^lvl,
 * corr [n, 7, 7, h1, w1].  h2, w2 are the LEVEL-0 target map sizes (the level's planes are (h2 >> lvl) x (w2 >> lvl)).
 * Bit-identical to dba_corr_index_forward on the reference-layout level; the adapter keeps a flow-aligned shadow of a
 * reference-layout level it is asked about repeatedly and serves the lookups from it (droid_backends/__init__.py). */
int dba_corr_lookup_level_sheared(const void *sheared_level, const float *coords_n2hw_scaled, void *corr, int n, int h1,
                                  int w1, int h2, int w2, int lvl, int radius, dba_stream_t stream);

/* the same on a slot-addressed shadow store (slots[e]: where edge e of the call lives), and the re-layout pass that fills
 * it: edge e of the pass is edge src_idx[e] of ref_level and goes to slot dst_slots[e] (either NULL: e).  Used by the
 * adapter when it matches the edges of a NEW reference-layout tensor (torch.cat / boolean index of the previous one:
 * dbaf/modules/corr.py:52-60) to shadows it already holds and re-lays only the edges it has not seen. */
int dba_corr_lookup_level_sheared_slots(const void *sheared_store, const int *slots, const float *coords_n2hw_scaled,
                                        void *corr, int n, int h1, int w1, int h2, int w2, int lvl, int radius,
                                        dba_stream_t stream);
int dba_corr_shear_level_slots(const void *ref_level, void *sheared_store, const int *src_idx, const int *dst_slots, int n,
                               int h1, int w1, int h2l, int w2l, int lvl, dba_stream_t stream);

/* corr_index_backward (src/correlation_kernels.cu:73-124,157-185): adjoint of the lookup;
 * volume_grad [n,h1,w1,h2,w2] must be zero-initialised by the caller. f32 only. */
int dba_corr_index_backward(const float *coords, const float *corr_grad, float *volume_grad, int n,
                            int h1, int w1, int h2, int w2, int radius, dba_stream_t stream);

/* CorrBlock.corr + pyramid (corr.py:24-38, :63-71): fmap1, fmap2 [n,C,h,w] f16 ->
 * level l [n,h1,w1,h2>>l,w2>>l] f16 for l < num_levels.  corr = (f1/4)^T (f2/4), fp32 accumulate on
 * MFMA, rounded once to f16; levels l>0 = 2x2 average of the rounded level l-1 (F.avg_pool2d).
 * scratch: device bytes from dba_corr_volume_scratch_bytes (channels-last staging of the fmaps). */
size_t dba_corr_volume_scratch_bytes(int n, int C, int h1, int w1, int h2, int w2);
int dba_corr_volume_build(const void *fmap1, const void *fmap2, void *const *levels /* host array */,
                          int n, int C, int h1, int w1, int h2, int w2, int num_levels, void *scratch,
                          size_t scratch_bytes, dba_stream_t stream);

/* altcorr_forward (src/droid.cpp:254-264, src/altcorr_kernel.cu:27-149,290-319): on-the-fly
 * windowed correlation. fmap1 [B,H1,W1,C], fmap2 [B,H2,W2,C] channels-last f32,
 * coords [B,S,H1,W1,2] f32 -> corr [B,S,(2r+1)^2,H1,W1] f32, channel = y_offset + (2r+1)*x_offset. */
int dba_altcorr_forward(const float *fmap1, const float *fmap2, const float *coords, float *corr, int B,
                        int S, int H1, int W1, int H2, int W2, int C, int radius, dba_stream_t stream);
/* the same with the element type of fmap1, fmap2 and corr selectable (the reference dispatches
 * AT_DISPATCH_FLOATING_TYPES_AND_HALF, src/altcorr_kernel.cu:304): dtype = DBA_F32 or DBA_F16; coords stay f32.
 * The half instantiation rounds every product and sum to half like c10::Half and is bit-identical to the reference. */
int dba_altcorr_forward_t(const void *fmap1, const void *fmap2, const float *coords, void *corr, int B, int S,
                          int H1, int W1, int H2, int W2, int C, int radius, int dtype, dba_stream_t stream);

/* AltCorrBlock.corr_fn (dbaf/modules/corr.py:107-125) in ONE launch: for every edge n (source frame ii[n], target frame
 * jj[n]; NULL = frame n), coordinate set and pyramid level l < num_levels, the on-the-fly correlation of fmap1 [F,H1,W1,C]
 * (level 0 of the pyramid) with fmap2_levels[l] [F,H1>>l,W1>>l,C] at coords / 2^l; corr [B,S,num_levels*(2r+1)^2,H1,W1].
 * Same arithmetic as dba_altcorr_forward_t per level (bit-identical), no gathered copies of the maps, no scaled copies of the
 * coordinates.  B * S * num_levels <= 65535. */
int dba_altcorr_pyramid_forward(const void *fmap1, const void *const *fmap2_levels /* host array of L device ptrs */,
                                const int64_t *ii, const int64_t *jj, const float *coords, void *corr, int B, int S, int H1,
                                int W1, int C, int num_levels, int radius, int dtype, dba_stream_t stream);

/* The same lookup for HALF feature pyramids with float output, on the matrix cores: what AltCorrBlock computes in the
 * reference, whose half pyramid (fmaps / 4 under autocast) is cast with .float() at every lookup (dbaf/modules/corr.py:120)
 * and correlated in float.  Products of halves are exact in float; the result differs from the float chain of
 * altcorr_kernel.cu:58-147 only in the order of the float additions.  fmap1 / fmap2_levels: half, channels-last
 * [F, H1 >> l, W1 >> l, C]; C % 16 == 0, C <= 128; radius 3; corr: float [B, S, L * 49, H1, W1]. */
int dba_altcorr_pyramid_forward_f16maps(const void *fmap1, const void *const *fmap2_levels /* host array of L device ptrs */,
                                        const int64_t *ii, const int64_t *jj, const float *coords, float *corr, int B, int S,
                                        int H1, int W1, int C, int num_levels, int radius, dba_stream_t stream);

/* altcorr_backward (src/droid.cpp:266-278, src/altcorr_kernel.cu:152-286,321-356; training only):
 * gradients wrt the feature maps; fmap1_grad [B,H1,W1,C], fmap2_grad [B,H2,W2,C] must be zero-initialised
 * by the caller (fmap2_grad is accumulated with float atomics like the reference); the reference's
 * coords_grad is allocated and never written (stays zero), so it has no entry point here. */
int dba_altcorr_backward(const float *fmap1, const float *fmap2, const float *coords, const float *corr_grad,
                         float *fmap1_grad, float *fmap2_grad, int B, int S, int H1, int W1, int H2, int W2,
                         int C, int radius, dba_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Geometry.
 * ---------------------------------------------------------------------------------------- */

/* pops.projective_transform without jacobians (dbaf/geom/projective_ops.py:96-125) as one kernel:
 * intrinsics [B,4] per frame; coords [N,ht,wd,2], valid [N,ht,wd,1] f32. */
int dba_reproject(const float *poses, const float *disps, const float *intrinsics_b4,
                  const int64_t *ii, const int64_t *jj, int N, int ht, int wd, float *coords,
                  float *valid, dba_stream_t stream);

/* droid_backends.frame_distance (src/droid.cpp:181-197, src/droid_kernels.cu:562-702). dist [N]. */
int dba_frame_distance(const float *poses, const float *disps, const float *intrinsics,
                       const int64_t *ii, const int64_t *jj, int N, int ht, int wd, float beta,
                       float *dist, dba_stream_t stream);

/* droid_backends.projmap (src/droid.cpp:200-215, src/droid_kernels.cu:471-560).
 * coords [N,ht,wd,3] (3rd channel left 0), valid [N,ht,wd,1]. */
int dba_projmap(const float *poses, const float *disps, const float *intrinsics, const int64_t *ii,
                const int64_t *jj, int N, int ht, int wd, float *coords, float *valid,
                dba_stream_t stream);

/* droid_backends.iproj (src/droid.cpp:218-227, src/droid_kernels.cu:824-895). points [nm,ht,wd,3]. */
int dba_iproj(const float *poses, const float *disps, const float *intrinsics, int nm, int ht, int wd,
              float *points, dba_stream_t stream);

/* droid_backends.depth_filter (src/droid.cpp:281-295, src/droid_kernels.cu:706-820).
 * counter [num,ht,wd] zero-initialised by the caller; nbuf = disps.size(0). */
int dba_depth_filter(const float *poses, const float *disps, const float *intrinsics,
                     const int64_t *inds, const float *thresh, int num, int nbuf, int ht, int wd,
                     float *counter, dba_stream_t stream);

/* ---- optional exchange step of the edge-sharded driver: one-shot all-reduce by direct peer reads ------------------
 * The reference is single-GPU (nothing to replace); SURVEY.md 8(e) asks for the float64 sum of the reduced camera
 * system [H | b] over the ranks, which dbaf_amd/sharded.py does with RCCL by default.  These entry points are the
 * latency-oriented alternative for one node (csrc/peer_allreduce.hip): every rank owns an exchange region that its
 * peers map through hipIpc and sums the world's contributions itself, in rank order (bit-identical replicas).
 *   bytes   = dba_peer_exchange_bytes(max_doubles)
 *   create  : hipMalloc + zero + IPC handle (64 bytes) of this rank's region
 *   open    : map a PEER process' region from its handle (not the creator's own: use the pointer `create` returned)
 *   close   : opened != 0 -> hipIpcCloseMemHandle, else hipFree
 *   allreduce: buf[0..n) += everybody else's, in place, enqueued on `stream`; `regions[world]` are device pointers (own
 *             region at index `rank`), `epoch` = 1, 2, 3, ... identical on all ranks and increasing by one per call,
 *             `status` a device int the kernel sets to DBA_PEER_TIMEOUT if a peer's contribution did not arrive within
 *             ~2 s (buf is left untouched then). */
/* ---- the `--upsample` path (csrc/upsample.hip) -------------------------------------------------------------------
 * convex upsampling of inverse depth: cvx_upsample with dim == 1 (dbaf/droid_net.py:17-31), called by
 * DepthVideo.upsample (dbaf/depth_video.py:205-209) as disps_up[ix] = cvx_upsample(disps[ix], mask).
 *   disps     [n_disps,ht,wd] f32;   mask [B,576,ht,wd] DBA_F32 or DBA_F16, channel = k*64 + a*8 + b with the 3x3 tap
 *             k = ky*3+kx reading disps[y+ky-1, x+kx-1] (zero outside the map);
 *   out       [n_out,8ht,8wd] f32 (16-byte aligned): out[dst, 8y+a, 8x+b] = sum_k softmax_k(mask[f,k*64+a*8+b,y,x]) * tap_k;
 *   src_rows, dst_rows [B] int64 device row maps of mask frame f (NULL = identity); frames whose rows fall outside
 *             [0,n_disps) / [0,n_out) are skipped.  A half mask rounds every weight to half before the product
 *             (torch.softmax keeps the mask's dtype), the sum is float. */
int dba_cvx_upsample_disp(const float *disps, int n_disps, const int64_t *src_rows, const void *mask, int mask_dtype,
                          int B, int ht, int wd, float *out, int n_out, const int64_t *dst_rows, dba_stream_t stream);
/* deterministic segmented sum / mean: torch_scatter.scatter_sum / scatter_mean with a 1-D index (dbaf/droid_net.py:14,65
 * GraphAgg; dbaf/geom/ba.py:7).  src [outer,n,inner] dtype (DBA_F32 / DBA_F16), index [n] int64 ->
 * out [outer,dim_size,inner]: out[o,s,i] = sum over e with index[e] == s of src[o,e,i], in ascending e, accumulated in
 * float and rounded once; mean != 0 divides by max(count_s, 1).  Every element of out is written (empty slots = 0);
 * index entries outside [0,dim_size) are ignored.  No atomics: bit-identical run to run. */
int dba_segment_reduce(const void *src, int dtype, const int64_t *index, int n, int64_t outer, int64_t inner,
                       int dim_size, int mean, void *out, dba_stream_t stream);
/* ---- upsample mode without the mask in HBM and without torch.unique (csrc/upmask.hip) ----------------------------
 * dba_upmask_upsample_disp: GraphAgg's `upmask = self.upmask(net)` (dbaf/droid_net.py:55-72, the 1x1 convolution of :70)
 *   and DepthVideo.upsample (dbaf/depth_video.py:205-209) with its cvx_upsample (dbaf/droid_net.py:17-31) in ONE launch:
 *   out[dst[f]] = cvx_upsample(disps[src[f]], W x[f] + b).  Half only.
 *     x        [B,128,ht,wd] half: the hidden state after conv2 and its ReLU;
 *     weight   [576,128] half (16-byte aligned), bias [576] half or NULL: the 1x1 convolution's parameters;
 *     disps    [n_disps,ht,wd] f32; out [n_out,8ht,8wd] f32 (16-byte aligned); src_rows, dst_rows [B] int64 or NULL
 *              (identity); frames whose rows fall outside the buffers are skipped;
 *     mask_out [B,576,ht,wd] half or NULL: receives the mask as the stock convolution would store it (the float sum plus
 *              the bias in float, rounded once), for every frame, skipped or not.  Must not overlap x.
 *   The product runs on mfma_f32_16x16x32_f16; the softmax and the weighted sum are the arithmetic of
 *   dba_cvx_upsample_disp on a half mask (one shared routine): fed this launch's mask_out, that entry point gives the same
 *   bits.  No atomics, no host synchronisation, no allocation.
 * dba_frame_plan: `uniq, inverse = torch.unique(ii, return_inverse=True)` (dbaf/droid_net.py:57 in GraphAgg.forward,
 *   :55-72) in one launch of one workgroup.  ii [n] int64, buffer <= dba_frame_plan_max_rows() rows; uniq [cap] int64,
 *   cap >= min(n, buffer): the distinct entries ascending, then -1; inverse [n] int64 (-1 for an entry outside
 *   [0, buffer)); res [4] device ints: n_uniq, the number of entries outside [0, buffer), the first such position (-1:
 *   none), 0.  expect >= 0: the n_uniq the caller sized its results for without reading `res`; if the launch finds
 *   another, or an entry out of range, it raises pinned host words that dba_frame_plan_poll returns (and clears) as
 *   out6 = {n_uniq, bad, first, expect, 0, -1}; poll touches no device. */
int dba_upmask_upsample_disp(const void *x, const void *weight, const void *bias, const float *disps, int n_disps,
                             const int64_t *src_rows, int B, int ht, int wd, float *out, int n_out,
                             const int64_t *dst_rows, void *mask_out, dba_stream_t stream);
int dba_frame_plan_max_rows(void);
int dba_frame_plan(const int64_t *ii, int n, int buffer, int cap, int64_t *uniq, int64_t *inverse, int *res, int expect,
                   dba_stream_t stream);
int dba_frame_plan_poll(int *out6);

/* ---- edge management of the covisibility graph (csrc/proximity.hip) ---------------------------------------------
 * dba_frame_distance_bidir: DepthVideo.distance with bidirectional=True (dbaf/depth_video.py:240-270) in one launch:
 *   dist[n] = .5f * (fd(ii[n],jj[n]) + fd(jj[n],ii[n])) in float, fd = dba_frame_distance's per-pair arithmetic, so the
 *   result is bit-identical to two dba_frame_distance calls averaged in float32 (:255-261).  Pairs with an index outside
 *   [0, n_frames) get NaN (nothing is read for them); n_frames = rows of poses and disps that may be read.
 * dba_proximity_edges: CovisibleGraph.add_proximity_factors (dbaf/covisible_graph.py:357-441) up to its add_factors
 *   call: the edge list es (:395-438), in the reference's order, for t = video.counter.value.  Candidates are
 *   meshgrid(arange(t0,t), arange(t1,t)) row-major (cc = (t-t0)(t-t1)), then the skip extras (t-1, t0+s) for each s of
 *   skip_edge_host[n_skip] with t0+s > 0 when (t-1) - t0 == frontend_window - 1 (:371-377).  Existing edges ex_ii/ex_jj
 *   [n_ex] = cat(ii, ii_bad, ii_inac), cat(jj, jj_bad, jj_inac) (:383-384).  Distances use beta (:379); selection follows
 *   :380-438 with thresh compared in double in the greedy pass (:412, d[k].item() > thresh) and in float32 for the skip
 *   tail (:436); argsort ties go to the lower candidate index, NaN sorts after +inf.
 *     dist   [cc + n_skip] f32 out: the candidates' distances after :380-381 (inf where ii - rad < jj, not computed, and
 *            where d > 100), the extras after the grid;
 *     edges  [2, capacity] int64 out: edges[0, 0..count) = ii, edges[1, 0..count) = jj;
 *     count  one device int: the edge count, -1 if capacity was too small, -2 where the reference raises IndexError (a
 *            stereo index below -len(d), :399).
 *   capacity >= dba_proximity_edges_capacity(t, t0, rad, stereo, max_factors) = step 4's edges + max(max_factors,0) + 4.
 *   Requires 0 <= t0 < t and 0 <= t1 < t; cc + n_skip > 8192 or n_skip > 16 is DBA_ERR_UNSUPPORTED.  Two launches.
 * dba_filter_repeated_edges: CovisibleGraph.__filter_repeated_edges (dbaf/covisible_graph.py:61-72): out = the
 *   proposals (ii, jj)[n] not in the existing list ex_ii/ex_jj [n_ex] = cat(ii, ii_inac), cat(jj, jj_inac), in order;
 *   duplicates inside the proposals are kept, as the reference keeps them.  out_ii/out_jj [n], *count = kept edges.
 * None of the three synchronises; none uses atomics (bit-identical run to run). */
int dba_frame_distance_bidir(const float *poses, const float *disps, const float *intrinsics, const int64_t *ii,
                             const int64_t *jj, int N, int n_frames, int ht, int wd, float beta, float *dist,
                             dba_stream_t stream);
int dba_proximity_edges_capacity(int t, int t0, int rad, int stereo, int max_factors);
int dba_proximity_edges(const float *poses, const float *disps, const float *intrinsics, int ht, int wd, int t,
                        int t0, int t1, int rad, int nms, float beta, double thresh, int max_factors, int stereo,
                        const int *skip_edge_host, int n_skip, int frontend_window, const int64_t *ex_ii,
                        const int64_t *ex_jj, int n_ex, float *dist, int64_t *edges, int capacity, int *count,
                        dba_stream_t stream);
int dba_filter_repeated_edges(const int64_t *ii, const int64_t *jj, int n, const int64_t *ex_ii, const int64_t *ex_jj,
                              int n_ex, int64_t *out_ii, int64_t *out_jj, int *count, dba_stream_t stream);

/* ---- retiring edges and dropping a keyframe (csrc/factors.hip) ---------------------------------------------------
 * The caller's edge bookkeeping around the update: CovisibleGraph.rm_factors (dbaf/covisible_graph.py:152-176),
 * rm_keyframe (:180-211), the frontend's retirement rule (dbaf/dbaf_frontend.py:235-239) and the edge statements of
 * __rollup (dbaf/dbaf_frontend.py:106-117).  Integers and bytes only: every result is exact.
 * dba_select_edges: one launch, one workgroup.  Decides for each edge p of (ii, jj, age)[n] whether it is dropped:
 *     DBA_SEL_MASK      mask[p] != 0                                  (rm_factors' mask, one byte per edge)
 *     DBA_SEL_RULE_OR   age > a  ||  (ii < b || jj < b)               (dbaf_frontend.py:238-239, a = max_age,
 *     DBA_SEL_RULE_AND  age > a  &&  (ii < b || jj < b)                :235-236         b = t1 - active_window)
 *     DBA_SEL_KEYFRAME  ii == a || jj == a, tested on the values as given; then every written entry >= a is
 *                       decremented (covisible_graph.py:197-199, :207-210)
 *     DBA_SEL_ROLL      ii - a < 0 || jj - a < 0; written entries are ii - a, jj - a (dbaf_frontend.py:108-112)
 *     DBA_SEL_SHIFT     nothing is dropped; written entries are ii - a, jj - a (:106-107, :117-118)
 *   and compacts both sides in the input's order (ballot + prefix sums, no atomics):
 *     keep [3, n] int64 out: rows ii, jj, age of the kept edges (the age row is left alone when age == NULL);
 *     drop [2, n_pre + n] int64 out: pre_ii / pre_jj [n_pre] copied to the front (rm_factors' torch.cat with the
 *          inactive lists, :158-159), then ii, jj of the dropped edges;
 *     sel  [2 + 2n] int32 out: n_keep, n_drop, the kept positions (n slots), the dropped positions (n slots): what the
 *          host reads, in one copy, to size the results; sel + 2 and sel + 2 + n are position lists for dba_move_rows.
 *   n > 8192 is DBA_ERR_UNSUPPORTED; n == 0 writes the two counts and copies pre.
 * dba_move_rows: ONE launch that executes up to DBA_MAX_ROW_JOBS row copies
 *     dst[(dst_row0 + r) * row_bytes ..] = src[(pos ? pos[r] : r) * row_bytes ..],  r in [0, count)
 *   for payloads of different row sizes; a position outside [0, src_rows) copies nothing.  Each job moves with the
 *   widest of 16 / 8 / 4 / 2 / 1 bytes that divides row_bytes and both base addresses.  Source and destination must
 *   not overlap.  dst_row0 + count <= dst_rows is checked on the host.
 * dba_shift_rows: ONE launch doing buf[ix] = buf[ix + 1] for up to DBA_MAX_SHIFT_BUFS buffers bases[k] of rows[k]
 *   rows of row_bytes[k] bytes (rm_keyframe's nine statements, covisible_graph.py:185-195); needs 0 <= ix < rows - 1.
 * The job and buffer tables are host arrays, passed to the kernel by value.  None of the three synchronises. */
#define DBA_SEL_MASK 0
#define DBA_SEL_RULE_OR 1
#define DBA_SEL_RULE_AND 2
#define DBA_SEL_KEYFRAME 3
#define DBA_SEL_ROLL 4
#define DBA_SEL_SHIFT 5
#define DBA_SEL_MAX_EDGES 8192
#define DBA_MAX_ROW_JOBS 8
#define DBA_MAX_SHIFT_BUFS 12
typedef struct dba_row_job {
  const void *src;    /* device: first source row */
  void *dst;          /* device: first destination row */
  const int *pos;     /* device: count source positions, or NULL for rows 0..count-1 */
  int64_t row_bytes;
  int count, dst_row0, src_rows, dst_rows;
} dba_row_job;
int dba_select_edges(const int64_t *ii, const int64_t *jj, const int64_t *age, int n, int mode,
                     const unsigned char *mask, int64_t a, int64_t b, const int64_t *pre_ii, const int64_t *pre_jj,
                     int n_pre, int64_t *keep, int64_t *drop, int *sel, dba_stream_t stream);
int dba_move_rows(const dba_row_job *jobs_host, int n_jobs, dba_stream_t stream);
int dba_shift_rows(void *const *bases_host, const int64_t *row_bytes_host, const int64_t *rows_host, int n_bufs,
                   int64_t ix, dba_stream_t stream);

/* ---- window rollup (csrc/rollup.hip) ----------------------------------------------------------------------------------
 * The torch.roll(x, -roll, 0) statements of DBAFusionFrontend.__rollup over the video buffers
 * (dbaf/dbaf_frontend.py:94-105) IN PLACE, and the `-= roll` of video.cur_ii / cur_jj (:121-122), in ONE launch with no
 * scratch buffer and no host read.  Up to DBA_MAX_SHIFT_BUFS buffers bases[k] of rows[k] rows of row_bytes[k] bytes, any
 * dtype and row size; up to DBA_MAX_ROLL_LISTS device int64 lists lists[k] of list_lens[k] entries, each entry minus roll.
 *   live < 0  (exact): every buffer becomes byte-identical to torch.roll(x, -roll, 0), new[r] = old[(r + roll) mod rows];
 *     roll is any integer, reduced mod rows[k] per buffer as torch does; a buffer whose reduced roll is 0 (or that has no
 *     rows or no bytes per row) is left out of the grid.
 *   live >= 0 (live rows only): new[r] = old[r + roll] for 0 <= r < live - roll, every other row untouched; needs
 *     0 <= roll <= live <= rows[k] for every buffer.  For the caller who knows that rows at or past `live` hold no frame.
 * The rows r, r + roll, r + 2 roll, ... form gcd(rows, roll) disjoint cycles (live: min(roll, live - roll) open chains); a
 * lane owns one such walk of one column element (the widest of 16 / 8 / 4 / 2 / 1 bytes dividing the base address and the
 * row size) and is the only thread that touches those bytes, eight rows in flight before the first store.
 * DBA_ERR_ARG before anything is enqueued: a null base with rows and bytes, a negative size, n_bufs > DBA_MAX_SHIFT_BUFS,
 * n_lists > DBA_MAX_ROLL_LISTS, a live-mode range violation, a grid past 2^31 - 1 workgroups.  A call with nothing to move
 * launches nothing.  The tables are host arrays, passed to the kernel by value.  Does not synchronise. */
#define DBA_MAX_ROLL_LISTS 4
int dba_roll_rows(void *const *bases_host, const int64_t *row_bytes_host, const int64_t *rows_host, int n_bufs, int64_t roll,
                  int64_t live, int64_t *const *lists_host, const int64_t *list_lens_host, int n_lists, dba_stream_t stream);

/* ---- adding edges (csrc/add_factors.hip) ----------------------------------------------------------------------------
 * CovisibleGraph.add_factors (dbaf/covisible_graph.py:102-149) in two launches around one host read.
 * dba_add_factors_plan: one launch, one workgroup, no atomics.  From the active lists (ii, jj, age)[n], the inactive
 *   lists (ii_inac, jj_inac)[n_inac] and the proposal (prop_ii, prop_jj)[n_prop]:
 *     filter   the proposals in neither list, in order, duplicates inside the proposal kept (:61-72); n_new of them
 *     evict    when n_new > 0 && may_evict && max_factors > 0 && n + n_new > max_factors (:118-119; may_evict = `remove`
 *              and a standing corr): mask[k] = argsort(age)[k] >= max_factors - n_new over POSITIONS k (:121-122), the
 *              argsort stable (ties to the lower position); a negative limit drops everything
 *     lists    [3, n + n_prop] int64 out: rows ii, jj, age; the kept edges in order, then the new ones with age 0;
 *              n_keep + n_new entries of each row are written (:141-143, :163-165)
 *     inac     [2, n_inac + n] int64 out, written only on eviction: the inactive lists, then the dropped edges (:157-158)
 *     info     [DBA_AF_INFO_WORDS + 2 n + 3 n_prop] int32 out, what the host reads in one copy: n_new, n_keep, n_drop,
 *              the verdict, 1 if the eviction ran, three spare words; then the kept positions (n slots) and the dropped
 *              positions (n slots), position lists as dba_move_rows takes them; then n_prop slots each of the source
 *              rows of the gathers: ii_new (nets, inps), ii_new * cams and jj_new * cams + (ii_new == jj_new) (fmaps
 *              [n_frames, cams, ...] viewed as rows, :128-130)
 *   verdict: 0, or DBA_AF_BAD_RANGE when a kept proposal has an index outside [0, n_frames), or DBA_AF_BAD_STEREO when
 *   a kept (i, i) needs a second camera and cams < 2 (the reference raises IndexError at :130).  The source rows of
 *   such an edge are written as -1, which the payload launch skips; the caller is expected to stop on a verdict.
 *   Any of n, n_inac, n_prop > 8192 is DBA_ERR_UNSUPPORTED.
 * dba_add_factors_payload: ONE launch that executes up to DBA_AF_MAX_JOBS row jobs
 *     DBA_AF_COPY       dst[dst_row0 + r] = src[r]                    (the inactive store in front of what it gains)
 *     DBA_AF_GATHER     dst[dst_row0 + r] = src[pos[r]]               (kept rows, dropped rows, nets[ii], fmaps[ii, 0] ...)
 *     DBA_AF_ZERO       dst[dst_row0 + r] = 0                         (the new weight rows, :139)
 *   r in [0, count), rows moved as dba_move_rows moves them (the same body and vector widths; a position outside
 *   [0, src_rows) copies nothing), and at most one
 *     DBA_AF_REPROJECT  dst[dst_row0 + e] = the coordinates of dba_reproject for edge (geom->ii[e], geom->jj[e]), bit for
 *                       bit, rows of [ht, wd, 2] float32 (:138); an edge with an index outside [0, geom->n_frames) writes
 *                       nothing
 *   The tables are host arrays, passed to the kernel by value.  Neither call synchronises. */
#define DBA_AF_INFO_WORDS 8
#define DBA_AF_BAD_RANGE 1
#define DBA_AF_BAD_STEREO 2
#define DBA_AF_MAX_JOBS 16
#define DBA_AF_COPY 0
#define DBA_AF_GATHER 1
#define DBA_AF_ZERO 2
#define DBA_AF_REPROJECT 3
typedef struct dba_af_job {
  int kind, reserved;
  dba_row_job rows; /* src unused by ZERO and REPROJECT, pos used by GATHER only */
} dba_af_job;
typedef struct dba_af_geometry {
  const float *poses;         /* device [n_frames, 7] */
  const float *disps;         /* device [n_frames, ht, wd] */
  const float *intrinsics_b4; /* device [n_frames, 4] */
  const int64_t *ii, *jj;     /* device: the edges of the REPROJECT job */
  int n_frames, ht, wd, reserved;
} dba_af_geometry;
int dba_add_factors_plan(const int64_t *ii, const int64_t *jj, const int64_t *age, int n, const int64_t *ii_inac,
                         const int64_t *jj_inac, int n_inac, const int64_t *prop_ii, const int64_t *prop_jj, int n_prop,
                         int max_factors, int may_evict, int n_frames, int cams, int64_t *lists, int64_t *inac,
                         int *info, dba_stream_t stream);
int dba_add_factors_payload(const dba_af_job *jobs_host, int n_jobs, const dba_af_geometry *geom_host,
                            dba_stream_t stream);

/* ---- the VIO update's BA inputs (csrc/update_inputs.hip) ------------------------------------------------------------
 * What CovisibleGraph.update(use_inactive=True) computes between the update operator and video.ba
 * (dbaf/covisible_graph.py:229-230, :242-247, :311-333), and the four .item() reads of DepthVideo.ba
 * (dbaf/depth_video.py:327-348), in two launches and no host synchronisation of their own.
 * dba_update_inputs_edges: one launch, one workgroup, no atomics.  From the inactive lists (ii_inac, jj_inac)[n_inac], the
 *   active lists (ii_act, jj_act)[n_act >= 1] and poses [n_frames, 7]:
 *     t0       has_t0 ? t0 : max(1, min(ii_act) + 1)                                                      (:229-230)
 *     sel      [n_inac] int32 out: the positions p with ii_inac[p] >= t0 - inac_range && jj_inac[p] >= t0 - inac_range,
 *              in list order (:243); n_sel of them
 *     ii_out, jj_out [n_inac + n_act] int64 out: the selected inactive edges, then the active ones (:244-245);
 *              N = n_sel + n_act entries are written
 *     kx       [min(n_frames, n_inac + n_act)] int64 out: torch.unique(ii_out), n_kx entries (:330)
 *     flags    [n_inac + n_act] bytes out, N written: bit 0 baseline_rule && ||(T_i * T_j^-1).t|| < mask_threshold with
 *              T = SE3(poses[.]), float32 in the operation order of the lietorch shim (:317-321); bit 1
 *              ii_out[e] == max(ii_out) (:327); bit 2 jj_out[e] == max(jj_out) (:328)
 *     res      [DBA_UI_RES_WORDS] int32 out: t0, n_sel, N, n_kx, min(ii_out), max(ii_out), min(jj_out), max(jj_out),
 *              and [8] = 1 when an index lies outside [0, n_frames) (such an edge gets no baseline flag and no row in kx)
 *   n_inac, n_act > 8192 or n_frames > DBA_UI_MAX_FRAMES is DBA_ERR_UNSUPPORTED; n_act == 0 is DBA_ERR_ARG.
 *   Called alone it serves as the count query: res is all a host needs to size the outputs.
 * dba_update_inputs_payload: one launch over (output edge, pixel chunk) and (damping row, pixel chunk).  target / weight
 *   rows [n, ht, wd, 2] f32 of the inactive and active tensors -> the planar [exp_N, 2, ht, wd] rows of :332-333, target
 *   unchanged, weight through, in this order and one float32 rounding each (a division by a host scalar is, on the
 *   device, a product with the scalar's float32 reciprocal -- what torch's kernels do):
 *       far_rule && disps[ii_out[e], p] < far_threshold  -> w * (1/1000)        (:311-314)
 *       flags[e] & 1                                     -> w * (1/1000)        (:317-322)
 *       flags[e] & 2                                     -> w * (1/10)          (:327)
 *       flags[e] & 4                                     -> w * (1/4)           (:328)
 *   and damping_out[r] = 0.2f * damping[kx[r]] + ep, two roundings, r < exp_n_kx (:330).  exp_n_sel, exp_N, exp_n_kx are
 *   the counts the outputs were sized for (they fix the grid); the kernel compares them with res[1..3] as the edge pass
 *   of THIS call left them.  On a mismatch (or res[8]) it writes zero target and weight rows and damping = ep -- a ba
 *   call with zero weights changes nothing -- and raises a pinned host word; it reads and writes nothing outside
 *   [0, exp_N) / [0, exp_n_kx) rows.  Pointers must be 8-byte aligned; 16-byte loads and stores where ht * wd is a multiple
 *   of 4 and the pointers allow.
 * dba_update_inputs_payload_op: dba_update_inputs_payload with the ACTIVE rows taken from the update operator's outputs
 *   instead of (target_act, weight_act) -- the two statements in front of the ones above (:235-236):
 *       target = coords1 + delta.to(float)   one float32 rounding        weight = weight.to(float)
 *   coords1 [n_act, ht, wd, 2] f32; delta, weight_op [n_act, ht, wd, 2] in op_dtype = DBA_F32 or DBA_F16 (a float16 widens
 *   exactly; another dtype is DBA_ERR_UNSUPPORTED).  target_new, weight_new [n_act, ht, wd, 2] f32 out, pixel-interleaved:
 *   what the caller assigns to self.target / self.weight, the weight BEFORE any rule (the rules act on the concatenated
 *   copy).  The lane that made an active row's values carries them on into the planar rows and the weight rules.  The
 *   launch reads neither target_new nor weight_new, so they may be the tensors the NEXT lookup reads.  Inactive and
 *   damping rows, the guard and the planar outputs are those of dba_update_inputs_payload; target_new / weight_new depend
 *   on no count and are written for all n_act rows whatever the guard says (rows that outputs sized for other counts do not
 *   reach get workgroups of their own).  Alignment: every float32 pointer 8 bytes, delta / weight_op 8 bytes in float32
 *   and 4 in float16 (a pixel's pair); 16-byte loads and stores where ht * wd is a multiple of 4 and EVERY pointer, the
 *   float16 ones included (8 values = 4 pixels per lane), is 16-byte aligned, else the one-pixel path.
 * dba_update_inputs_poll: 1 when a payload pass reported a mismatch since the last poll (counts6 = the edge pass's n_sel,
 *   N, n_kx, then the expected three), else 0.  Reads pinned host memory: no device synchronisation. */
#define DBA_UI_MAX_FRAMES 1024
#define DBA_UI_RES_WORDS 16
int dba_update_inputs_edges(const int64_t *ii_inac, const int64_t *jj_inac, int n_inac, const int64_t *ii_act,
                            const int64_t *jj_act, int n_act, const float *poses, int n_frames, int has_t0, int64_t t0,
                            int64_t inac_range, float mask_threshold, int baseline_rule, int *sel, int64_t *ii_out,
                            int64_t *jj_out, unsigned char *flags, int64_t *kx, int *res, dba_stream_t stream);
int dba_update_inputs_payload(const float *target_inac, const float *weight_inac, int n_inac, const float *target_act,
                              const float *weight_act, int n_act, const float *disps, const float *damping,
                              int n_frames, int ht, int wd, float far_threshold, int far_rule, float ep, const int *sel,
                              const int64_t *ii_out, const unsigned char *flags, const int64_t *kx, const int *res,
                              int exp_n_sel, int exp_N, int exp_n_kx, float *target_out, float *weight_out,
                              float *damping_out, dba_stream_t stream);
int dba_update_inputs_payload_op(const float *target_inac, const float *weight_inac, int n_inac, const float *coords1,
                                 const void *delta, const void *weight_op, int op_dtype, int n_act, const float *disps,
                                 const float *damping, int n_frames, int ht, int wd, float far_threshold, int far_rule,
                                 float ep, const int *sel, const int64_t *ii_out, const unsigned char *flags,
                                 const int64_t *kx, const int *res, int exp_n_sel, int exp_N, int exp_n_kx,
                                 float *target_out, float *weight_out, float *damping_out, float *target_new,
                                 float *weight_new, dba_stream_t stream);
int dba_update_inputs_poll(int *counts6);

/* ---- the window split of the VIO update (csrc/vio_window.hip) -------------------------------------------------------
 * The statements of DepthVideo.ba's IMU branch that feed its two BACore.init calls (dbaf/depth_video.py:360-367, :388-390,
 * :470-475) in two launches and no host synchronisation of their own.  Integers and bytes only: every result is exact.
 * dba_vio_window_plan: one launch, one workgroup, no atomics.  Two selections, each compacted in list order:
 *     marginalised  over the old window's lists (cur_ii, cur_jj)[n_cur]: last_t0 <= ii < lo && ii < last_t1 - 2 &&
 *                   jj < last_t1 - 2 (:360-364); n_cur == 0: the branch is not entered, the marg_* outputs may be NULL
 *     active        over the call's lists (ii, jj)[n >= 1]: ii >= t0 && jj >= t0 (:470)
 *     marg_ii, marg_jj [n_cur], act_ii, act_jj [n] int64 out: the selected edges (:366-367, :471-472); behind the count the
 *                   input's own entries at those positions
 *     marg_pos [n_cur], act_pos [n] int32 out: the selected positions, position lists as dba_move_rows takes them; -1
 *                   behind the count
 *     res      [DBA_VW_RES_WORDS] int32 out: n_marg, max(marg_jj) (:372; -2^30 when nothing is selected), n_active,
 *              min(ii) over the whole list (:475); indices are clamped to +-2^30
 *   n_cur or n > 8192 is DBA_ERR_UNSUPPORTED; n == 0 is DBA_ERR_ARG.
 * dba_vio_window_payload: ONE launch that executes up to DBA_VW_MAX_JOBS gathers dst[dst_row0 + r] = src[pos[r]], r in
 *   [0, count), rows moved as dba_move_rows moves them (the same body and vector widths): marg_target, marg_weight
 *   (:388-389), cur_target, cur_weight (:473-474).  expect4_host = the four words of res the jobs' counts and the caller's
 *   eta views were taken from; the kernel compares them with res as the plan of THIS call left it.  On a mismatch every
 *   job's rows are zeroed -- BACore with zero weights has nothing to linearise -- and a pinned host word is raised; nothing
 *   outside the jobs' rows is written.  A call without rows still launches the comparison.
 * dba_vio_window_poll: 1 when a payload launch reported a mismatch since the last poll (words8 = the plan's four words,
 *   then the expected four), else 0.  Reads pinned host memory: no device synchronisation. */
#define DBA_VW_RES_WORDS 4
#define DBA_VW_MAX_JOBS 4
int dba_vio_window_plan(const int64_t *cur_ii, const int64_t *cur_jj, int n_cur, int64_t last_t0, int64_t lo,
                        int64_t last_t1, const int64_t *ii, const int64_t *jj, int n, int64_t t0, int64_t *marg_ii,
                        int64_t *marg_jj, int *marg_pos, int64_t *act_ii, int64_t *act_jj, int *act_pos, int *res,
                        dba_stream_t stream);
int dba_vio_window_payload(const dba_row_job *jobs_host, int n_jobs, const int *res, const int *expect4_host,
                           dba_stream_t stream);
int dba_vio_window_poll(int *words8);

/* ---- keyframe gating (csrc/keyframe.hip) ----------------------------------------------------------------------------
 * The two per-frame decisions the host takes from device data, each in ONE launch of one workgroup and ONE host wait.  The
 * launch writes a report into pinned, host-coherent 32-bit words owned by the library and then a completion word; the host
 * spins on that word (BACore.hessian's hand-over).  Neither the launches nor the wait synchronises the stream.
 * dba_keyframe_report_words: the words of a report, DBA_KF_WORDS.  Layout: [DBA_KF_D] d or the flow magnitude (float),
 *   [DBA_KF_WIN] the window length, 7 or 3 (int), [DBA_KF_CAM .. +7) cam_translation (float; 0 behind the window),
 *   [DBA_KF_MAT .. +16) the 4x4 matrix, row-major (float), [DBA_KF_SEQ] the completion word (int).
 * dba_keyframe_report: *report = the block of (current device, stream), allocated zeroed at first use and never freed while
 *   the process lives, *seq = its next sequence number (1, 2, ...).  A block serves one call at a time: a later launch
 *   overwrites it, so the host copies what it needs before it asks for the block again.
 * dba_keyframe_check: dbaf/dbaf_frontend.py:262-264 and :319-324 up to the host's comparisons.
 *     d    = DepthVideo.distance([t1-3], [t1-2], beta, bidirectional=True): lanes 0-255 and 256-511 run
 *            dba_frame_distance's per-pair arithmetic for (t1-3, t1-2) and (t1-2, t1-3); bit-identical to
 *            dba_frame_distance_bidir on that pair, the 1000 sentinel of a pair with < 75 % valid weight included;
 *     cam  = torch.norm((poses[k0:t1-3] * poses[t1-2].inv()[None]).translation()[:, 0:3], dim=1), k0 = t1-10 when
 *            t1 > 10, else t1-6: cam[k] = |qrot(q_k, t_inv) + t_k|, (t_inv, q_inv) = inv(poses[t1-2]);
 *     mat  = poses[t1-1].inv().matrix();
 *   cam and mat in float32 with unfused operations in the order of the lietorch shim's formulas.  poses [n_frames,7],
 *   disps [n_frames,ht,wd], intrinsics [4] f32.  Only pose rows [k0, t1) and disps rows t1-3, t1-2 are read.
 *   t1 < 6, t1 - 1 >= n_frames or ht * wd == 0 is DBA_ERR_ARG, as is a report that is not the stream's block.
 * dba_keyframe_flow_magnitude: delta.norm(dim=-1).mean() of dbaf/motion_filter.py:87: the mean over n_pixels (dx, dy)
 *   pairs of sqrt(dx^2 + dy^2), in word DBA_KF_D (the other payload words are left as they are).  One fixed summation
 *   order (lane-strided, wave sum, partials in wave order): bit-identical run to run.  DBA_F32: float throughout.
 *   DBA_F16: torch's half semantics -- each norm in float, rounded to half; the halves summed in float; the mean rounded
 *   to half.  delta aligned to one pair.  n_pixels == 0 is DBA_ERR_ARG; another dtype DBA_ERR_UNSUPPORTED.
 * dba_keyframe_wait: returns once the block's completion word shows seq.  Every few thousand looks it asks the runtime
 *   whether the block's stream has drained; drained without the word (a launch that failed) is DBA_ERR_HIP. */
#define DBA_KF_D 0
#define DBA_KF_WIN 1
#define DBA_KF_CAM 2
#define DBA_KF_MAT 9
#define DBA_KF_SEQ 25
#define DBA_KF_WORDS 26
int dba_keyframe_report_words(void);
int dba_keyframe_report(dba_stream_t stream, void **report, int *seq);
int dba_keyframe_check(const float *poses, const float *disps, const float *intrinsics, int n_frames, int ht, int wd,
                       int t1, float beta, void *report, int seq, dba_stream_t stream);
int dba_keyframe_flow_magnitude(const void *delta, int dtype, int n_pixels, void *report, int seq, dba_stream_t stream);
int dba_keyframe_wait(const void *report, int seq);

/* ---- ConvGRU glue (csrc/gru.hip) --------------------------------------------------------------------------------------
 * The body of ConvGRU.forward (dbaf/modules/gru.py:19-32) around its seven convolutions, which stay with the caller, in
 * four launches.  Tensors are [n, c, hw] of one dtype, DBA_F16 or DBA_F32 (another is DBA_ERR_UNSUPPORTED), aligned to an
 * element.  Every statement of the reference yields a tensor of that dtype: h(.) below rounds to it, and the arithmetic
 * between two roundings is float32, unfused.  Vectors of 16 bytes where the extents and the bases allow, else elements;
 * no atomics, no host read, one fixed summation order.  Each call refuses, without a launch and with DBA_ERR_ARG: an extent
 * <= 0, c * hw or n * c or the grid beyond 2^31 - 1, a null pointer, a destination that shares a byte with a source.
 * dba_gru_pack: dst [n, sum c_k, hw] = the n_src <= DBA_GRU_MAX_SOURCES sources [n, c_k, hw] one behind the other along the
 *   channels: inp = torch.cat(inputs, dim=1); net_inp = torch.cat([net, inp], dim=1) (:20-21) with srcs = (net, *inputs),
 *   written once, byte-exact.  srcs and channels are HOST arrays of n_src entries.
 * dba_gru_context: glo [n, c] = h(mean_hw(h(h(sigmoid(a)) * net))), a = w(net): glo = torch.sigmoid(self.w(net)) * net;
 *   glo.view(b, c, h*w).mean(-1) (:24-25).  The sum is float32, times the float32 1 / hw as torch's mean.
 * dba_gru_reset: buf [n, c_total, hw], channels [0, c) of every edge = h(h(sigmoid(h(cr + gr))) * net), cr = convr(net_inp)
 *   [n, c, hw], gr = convr_glo(glo) [n, c]: r = torch.sigmoid(self.convr(net_inp) + self.convr_glo(glo)) and the first half of
 *   torch.cat([r*net, inp], dim=1) (:28-29); channels [c, c_total) are not touched, so a buffer dba_gru_pack filled IS that
 *   cat afterwards.  Every reader of buf's old content (convz, convr) must have been enqueued before.
 * dba_gru_blend: out [n, c, hw] = h(h(h(1 - z) * net) + h(z * q)), z = h(sigmoid(h(cz + gz))), q = h(tanh(h(cq + gq))) (:27,
 *   :29, :31); cz, cq [n, c, hw], gz, gq [n, c].  out == net is allowed (in place), any other overlap is not. */
#define DBA_GRU_MAX_SOURCES 8
int dba_gru_pack(const void *const *srcs, const int *channels, int n_src, int n, int hw, int dtype, void *dst,
                 dba_stream_t stream);
/* dba_gru_pack with torch.relu applied to the sources whose bit of relu_mask is set (bit k: srcs[k]) while they are copied:
 * byte-equal to torch.cat of the sources with torch.relu on the marked ones (NaN goes through with its payload, -0 and
 * everything negative become +0).  A launch of its own kernel; relu_mask == 0 copies as dba_gru_pack does. */
int dba_gru_pack_relu(const void *const *srcs, const int *channels, int n_src, int n, int hw, int dtype, void *dst,
                      unsigned relu_mask, dba_stream_t stream);
int dba_gru_context(const void *a, const void *net, int n, int c, int hw, int dtype, void *glo, dba_stream_t stream);
int dba_gru_reset(void *buf, int c_total, const void *cr, const void *gr, const void *net, int n, int c, int hw, int dtype,
                  dba_stream_t stream);
int dba_gru_blend(const void *cz, const void *gz, const void *cq, const void *gq, const void *net, int n, int c, int hw,
                  int dtype, void *out, dba_stream_t stream);

/* ---- 3x3 convolutions on the matrix cores, with the ConvGRU's gates in the epilogue (csrc/conv3x3.hip) ------------------
 * nn.Conv2d(C_in, C_out, 3, padding=1) on half tensors [n, C, h, w]: implicit GEMM on mfma_f32_16x16x32_f16, float32
 * accumulation in one fixed order (no atomics: the same bits on every run), then c = half(acc + float(bias)), ONE rounding.
 *   input    C_in = c0 + c1 channels from two sources: channels [0, c0) are src0 [n, c0, h, w], channels [c0, c0 + c1) are
 *            the channels src1_first .. + c1 of src1 [n, c1_total, h, w].  c1 == 0: src0 alone (src1 is not read).
 *   weight   [9][C_out][C_in] half, tap-major (tap = 3 ky + kx): weight.permute(2, 3, 0, 1) of the module's [C_out, C_in, 3,
 *            3], 16-byte aligned.  bias [C_out] half or NULL.
 * dba_conv3x3_f16: out [n, c_out, h, w] = c, or torch.relu(c) when relu != 0.
 * dba_conv3x3_gates_f16: C_out = 2c, the weights and biases of convz then convr one behind the other; gz, gr [n, c], net
 *   [n, c, h, w].  z_out = h(sigmoid(h(c_z + gz))); rnet_out = h(h(sigmoid(h(c_r + gr))) * net): convz, convr and
 *   dba_gru_reset in one launch, with dba_gru_reset's and dba_gru_blend's statements (one shared routine).  Neither output
 *   may share a byte with an input: neighbouring workgroups read every input channel with a halo.
 * dba_conv3x3_blend_f16: C_out = c; gq [n, c], z, net [n, c, h, w].  out = h(h(h(1 - z) * net) + h(z * q)), q =
 *   h(tanh(h(c_q + gq))): convq and dba_gru_blend in one launch.  out == net is allowed, any other overlap is not.
 * Refused without a launch, DBA_ERR_ARG: c0 % 32, c1 % 32 or C_out % 64 not 0, an extent <= 0, src1_first + c1 > c1_total, a
 * null pointer, a weight that is not 16-byte aligned, h * w * channels of one image or the grid beyond 2^31 - 1, an output
 * that shares a byte with an input.  dba_conv3x3_tile: the side of a workgroup's square pixel tile. */
int dba_conv3x3_tile(void);
int dba_conv3x3_f16(const void *src0, int c0, const void *src1, int c1, int c1_total, int src1_first, const void *weight,
                    const void *bias, int c_out, int n, int h, int w, int relu, void *out, dba_stream_t stream);
int dba_conv3x3_gates_f16(const void *src0, int c0, const void *src1, int c1, int c1_total, int src1_first,
                          const void *weight, const void *bias, const void *gz, const void *gr, const void *net, int c, int n,
                          int h, int w, void *z_out, void *rnet_out, dba_stream_t stream);
int dba_conv3x3_blend_f16(const void *src0, int c0, const void *src1, int c1, int c1_total, int src1_first,
                          const void *weight, const void *bias, const void *gq, const void *z, const void *net, int c, int n,
                          int h, int w, void *out, dba_stream_t stream);
/* dba_conv3x3_pair_f16: C_out = 2c, the weights and biases of two convolutions of one input one behind the other (the heads'
 *   delta[0] then weight[0]).  out0 [n, c, h, w] = the channels [0, c) of c, out1 [n, c, h, w] the channels [c, 2c), each
 *   through torch.relu when relu != 0: byte for byte the two halves of dba_conv3x3_f16 on the same operands (same tile,
 *   staging and accumulation order), written as two contiguous tensors.  Refused as dba_conv3x3_f16 refuses, and when out0
 *   and out1 share a byte. */
int dba_conv3x3_pair_f16(const void *src0, int c0, const void *src1, int c1, int c1_total, int src1_first, const void *weight,
                         const void *bias, int c, int n, int h, int w, int relu, void *out0, void *out1, dba_stream_t stream);

/* ---- 3x3 convolution with the frame mean behind it (csrc/conv3x3_mean.hip) -----------------------------------------------
 * GraphAgg's `scatter_mean(relu(conv1(net)), ix, dim=1)` (dbaf/droid_net.py:57-65) in ONE launch: the [n, C_out, h, w] tensor
 * between dba_conv3x3_f16(relu = 1) and dba_segment_reduce(mean = 1, dim_size = F) is never written, and out has the bytes
 * of those two launches.
 * dba_frame_members: the member table of a plan.  inverse [n] int64 (dba_frame_plan's), F slots, 1 <= F <=
 *   dba_frame_members_max_slots(); seg_start [F + 1] int32, members [n] int32: members[seg_start[s] .. seg_start[s + 1]) are
 *   the edges e with inverse[e] == s, ascending (a stable counting sort, one launch of one workgroup, no atomics); entries of
 *   inverse outside [0, F) belong to no slot, as dba_segment_reduce ignores them; members behind seg_start[F] are -1.
 * dba_conv3x3_mean_f16: src [n, c_in, h, w] half, weight [9][c_out][c_in] and bias as dba_conv3x3_f16 takes them (one source),
 *   seg_start [F + 1], members [n] as dba_frame_members writes them, out [out_rows, c_out, h, w] half:
 *     out[s] = half(sum over the members e of slot s, ascending, of float(relu(half(conv(src[e]) + bias))) / float(max(count, 1)))
 *   for s < F, a float32 sum from 0 and an IEEE division; rows [F, out_rows) are not touched; an empty slot is zeros.
 *   out_rows is the number of [c_out, h, w] rows that `out` HOLDS, and F <= out_rows is checked here.  It exists because a
 *   launch writes F rows and a C caller's F says nothing about the buffer behind `out`: an earlier form of this entry took
 *   F alone, was called with F beyond its buffer and faulted the device.  A caller passes the row count of the allocation
 *   itself (dbaf_amd.conv.conv3x3_frame_mean passes out.shape[0]), never F again.
 *   Returns DBA_ERR_ARG BEFORE ANY HIP RUNTIME CALL when F < 1, F > out_rows, n < 1, an extent <= 0, src, weight, seg_start,
 *   members or out is null, c_in % 32 or c_out % 64 is not 0, weight is not 16-byte aligned (the tables 4-byte, the halves
 *   2-byte), h * w * channels of one image or the grid exceeds 2^31 - 1, or out[0 .. F) shares a byte with an input.
 *   Whatever the tables hold, the kernel reads seg_start[0 .. F], members[0 .. n) and rows [0, n) of src only: a slot's
 *   bounds are clamped to [0, n] and a member outside [0, n) is skipped. */
int dba_frame_members_max_slots(void);
int dba_frame_members(const int64_t *inverse, int n, int F, int *seg_start, int *members, dba_stream_t stream);
int dba_conv3x3_mean_f16(const void *src, int c_in, const void *weight, const void *bias, int c_out, int n, int h, int w,
                         const int *seg_start, const int *members, int F, void *out, int out_rows, dba_stream_t stream);

/* ---- 1x1 convolutions on the matrix cores, with the ConvGRU's context chain behind one (csrc/conv1x1.hip) ---------------
 * nn.Conv2d(C_in, C_out, 1) on half tensors [n, C, hw] (the plane flattened): a GEMM on mfma_f32_16x16x32_f16,
 *   c[n, o, p] = half(sum_i W[o, i] * x[n, i, p] + float(b[o])),
 * a float32 sum in one fixed order (chunks of 32 channels ascending, the hardware's order inside an MFMA; no atomics: the same
 * bits on every run), ONE rounding.  C_in is any positive count, C_out a multiple of 64.
 *   weight   [C_out][Kp] half, Kp = C_in rounded up to a multiple of 32, the columns [C_in, Kp) ZERO, 16-byte aligned.  bias
 *            [C_out] half or NULL.  No load touches an address outside x, weight and bias.
 * dba_conv1x1_f16: out [n, c_out, hw] = c, or torch.relu(c) when relu != 0 (NaN stays, -0 -> +0).
 * dba_conv1x1_context_f16: C_in = C_out = c <= 1024, weight / bias those of ConvGRU.w.  a = c above is never stored.
 *   glo [n, c] = h(sum_p(h(h(sigmoid(a)) * net)) * float32(1 / hw)), dba_gru_context's statement: glo = torch.sigmoid(self.w(net))
 *   * net; glo.view(b, c, h*w).mean(-1) (dbaf/modules/gru.py:24-25).  The float32 sum of a plane runs in ONE order: inside a tile
 *   of dba_conv1x1_tile() pixels a lane adds the pixels r, r + 16, .. ascending and 16 lanes fold by shifts of 1, 2, 4, 8; a
 *   second launch adds the tiles' partial sums (workspace, float32 [n, tiles, c]) in tile order.
 *   gz, gr, gq [n, c] = half(sum_i Wg[o, i] * float(glo[n, i]) + float(bg[o])) for the rows o of glo_weight [3c][c] (convz_glo,
 *   convr_glo, convq_glo one behind the other, 16-byte aligned) and glo_bias [3c] or NULL: a float32 sum over i ascending, ONE
 *   rounding (:27-29's convX_glo(glo)).  Two launches in all.  workspace: at least dba_conv1x1_context_workspace_bytes(n, c, hw)
 *   bytes, 4-byte aligned, else DBA_ERR_WORKSPACE.
 * Refused without a launch, DBA_ERR_ARG: an extent <= 0, C_out % 64 != 0, a null or misaligned pointer, hw * channels of one
 * image or the grid beyond 2^31 - 1, an output (or the workspace) that shares a byte with an input or with another output.
 * dba_conv1x1_tile: the pixels of a workgroup's tile. */
int dba_conv1x1_tile(void);
int dba_conv1x1_f16(const void *x, int c_in, const void *weight, const void *bias, int c_out, int n, int hw, int relu, void *out,
                    dba_stream_t stream);
size_t dba_conv1x1_context_workspace_bytes(int n, int c, int hw);
int dba_conv1x1_context_f16(const void *net, const void *weight, const void *bias, const void *glo_weight, const void *glo_bias,
                            int c, int n, int hw, void *workspace, size_t workspace_bytes, void *glo, void *gz, void *gr,
                            void *gq, dba_stream_t stream);

/* ---- 7x7 convolution of four channels on the matrix cores: the update operator's flow stem (csrc/conv7x7.hip) -----------
 * nn.Conv2d(4, C_out, 7, padding=3) on x [n, 4, h, w] (dbaf/droid_net.py:85-86): a GEMM on mfma_f32_16x16x32_f16 whose K is
 * one kernel row, 7 taps and one zero slot of 4 channels each,
 *   c[n, o, y, x] = half(sum_{i, ky, kx} W[o, i, ky, kx] * half(x[n, i, y + ky - 3, x + kx - 3]) + float(b[o])),
 * zeros outside the map; a float32 sum in one fixed order (kernel rows ky = 0 .. 6 ascending, the hardware's order inside an
 * MFMA; no atomics: the same bits on every run), ONE rounding.  C_in is 4 and nothing else, C_out a multiple of 64.
 *   x        dtype = DBA_F16 or DBA_F32, aligned to an element.  A float32 value is rounded to half as it is read (to nearest
 *            even, beyond 65504 to infinity): the bytes of x.to(torch.float16), without that launch.
 *   weight   [7][C_out][32] half, entry [ky][o][4 kx + i] = W[o, i, ky, kx] for kx < 7 and ZERO for kx = 7, 16-byte aligned.
 *            bias [C_out] half or NULL.  No load touches an address outside x, weight and bias.
 *   The eighth slot of a kernel row lies on the pixel right of the footprint; the kernel feeds the matrix core zeros there,
 *   so a NaN or an infinity of the input reaches exactly the outputs whose 7x7 window holds it.
 * dba_conv7x7_f16: out [n, c_out, h, w] half = c, or torch.relu(c) when relu != 0 (NaN stays, -0 -> +0).  One launch.
 * Refused without a launch, DBA_ERR_ARG: an extent <= 0, C_out % 64 != 0, a dtype other than the two, a null pointer (bias
 * excepted), a misaligned pointer, h * w * C_out of one image or the grid beyond 2^31 - 1, an output that shares a byte with
 * an input.
 * dba_conv7x7_tile: the side of a workgroup's square pixel tile. */
int dba_conv7x7_tile(void);
int dba_conv7x7_f16(const void *x, int dtype, const void *weight, const void *bias, int c_out, int n, int h, int w, int relu,
                    void *out, dba_stream_t stream);

/* ---- The encoders' convolutions on the matrix cores (csrc/conv_enc.hip) ------------------------------------------------
 * The 16 convolutions of BasicEncoder (dbaf/modules/extractor.py:10-11, :45, :136, :145) that conv3x3 / conv1x1 above do not take:
 * stride 2, C_out = 32, three input channels.  Half tensors [n, C, h, w]; implicit GEMM on mfma_f32_16x16x32_f16, float32
 * accumulation in one fixed order (no atomics: the same bits on every run), then c = half(acc + float(bias)), ONE rounding;
 * relu != 0: torch.relu(c) (NaN stays, -0 -> +0).  Positions outside the image are zeros and are never dereferenced.  The
 * output has oh = (h - 1) / stride + 1 rows and ow = (w - 1) / stride + 1 columns.
 * dba_conv3x3s_f16: nn.Conv2d(c_in, c_out, 3, stride=stride, padding=1)(x) (ResidualBlock.conv1 / conv2, extractor.py:10-11),
 *   stride 1 or 2, c_in % 32 == 0, c_out % 32 == 0.  weight [9][c_out][c_in] half, tap-major (tap = 3 ky + kx), 16-byte
 *   aligned; bias [c_out] half or NULL.  Order of an output element: chunks of 32 input channels ascending; inside a chunk
 *   kx = 0, 1, 2; inside kx ky = 0, 1, 2; inside an MFMA the hardware's order.  It does not depend on n, on the tile, or on
 *   how a workgroup's waves divide channels and rows (64 channels a workgroup where c_out % 64 == 0, else 32).
 * dba_conv3x3s_down_f16: a stride-2 block's conv1 and its downsample[0] = nn.Conv2d(c_in, c_out, 1, stride=2) (extractor.py:
 *   45) in one launch: downsample[0] reads input pixel (2y, 2x), the centre tap of conv1 at stride 2 with padding 1.
 *   weight [10][c_out][c_in]: conv1's nine slices, then the 1x1 weight [c_out][c_in].  out = dba_conv3x3s_f16's bytes at
 *   stride 2 (through the ReLU when relu != 0); out_down = half(sum_i Wd[o, i] * x[n, i, 2y, 2x] + float(bias_down[o])),
 *   chunks ascending, never through the ReLU.  Both [n, c_out, oh, ow].
 * dba_conv7x7s2_f16: the stem nn.Conv2d(3, c_out, 7, stride=2, padding=3)(x.half()) (extractor.py:136), c_out % 32 == 0.
 *   x [n, 3, h, w], dtype DBA_F16 or DBA_F32, aligned to an element; a float32 value is rounded to half as it is read (to
 *   nearest even, beyond 65504 to infinity): the bytes of x.to(torch.float16).  weight [7][c_out][32] half, entry [ky][o][4 kx
 *   + i] = W[o, i, ky, kx] for kx < 7 and i < 3, ZERO for kx = 7 and for i = 3, 16-byte aligned.  The kernel feeds the
 *   matrix core zeros in those slots too, so a NaN or an infinity of the input reaches exactly the outputs whose window
 *   holds it.  Order of an output element: kernel rows ky = 0 .. 6 ascending, the hardware's order inside an MFMA.
 * Refused without a launch, DBA_ERR_ARG: an extent <= 0, a stride other than 1 and 2, c_in % 32 or c_out % 32 not 0, a dtype
 * other than the two, a null pointer (a bias excepted), a misaligned pointer, h * w * channels of one image or the grid
 * beyond 2^31 - 1, an output that shares a byte with an input or with the other output.
 * dba_conv3x3s_tile_rows(stride) / dba_conv3x3s_tile_cols(): a workgroup's tile of OUTPUT pixels (16 x 16 at stride 1, 8 rows
 * x 16 columns at stride 2; 0 rows for another stride).  dba_conv7x7s2_tile: the side of the stem's square output tile. */
int dba_conv3x3s_tile_rows(int stride);
int dba_conv3x3s_tile_cols(void);
int dba_conv7x7s2_tile(void);
int dba_conv3x3s_f16(const void *x, const void *weight, const void *bias, int c_in, int c_out, int n, int h, int w, int stride,
                     int relu, void *out, dba_stream_t stream);
int dba_conv3x3s_down_f16(const void *x, const void *weight, const void *bias, const void *bias_down, int c_in, int c_out, int n,
                          int h, int w, int relu, void *out, void *out_down, dba_stream_t stream);
int dba_conv7x7s2_f16(const void *x, int dtype, const void *weight, const void *bias, int c_out, int n, int h, int w, int relu,
                      void *out, dba_stream_t stream);

/* ---- Encoder glue (csrc/extractor.hip) -----------------------------------------------------------------------------
 * What the feature and context encoders (dbaf/modules/extractor.py:47-55, :183-198) and their caller
 * (dbaf/motion_filter.py:29-30, :35-36, :64-65) run between the convolutions, which stay with the caller.  Tensors are
 * [planes, hw] contiguous of one dtype, DBA_F16 or DBA_F32 (another is DBA_ERR_UNSUPPORTED), aligned to an element.  Every
 * statement of the reference yields a tensor of that dtype: h(.) rounds to it, the arithmetic between two roundings is
 * float32, unfused.  relu(x) = x > 0 ? x : (x != x ? x : 0): NaN goes through, as torch.relu lets it.  16-byte accesses
 * where the extents and bases allow, else elements; no atomics, no host read, work on `stream` only.  Each call refuses,
 * without a launch and with DBA_ERR_ARG: a null pointer, an extent <= 0, a grid beyond 2^31 - 1, an overlap not named below.
 * norm(x)_i = (x_i - m) * r per plane: m = (sum x_i) / hw, r = 1 / sqrt(v + eps), v = (sum (x_i - m)^2) / hw over the values
 *   the workgroup holds (not E[x^2] - m^2), float32.  One workgroup holds one plane in registers, so hw <= 65536 (beyond:
 *   DBA_ERR_ARG).  A plane is n_items items, vectors of 16 bytes (hw * itemsize a multiple of 16 and every base aligned) or
 *   elements; lanes = the power of two >= n_items / 2 (elements: n_items / 4) within [64, 1024]; lane t holds items t,
 *   t + lanes, ... (per lane: the power of two >= n_items / lanes; elements: the next of 1, 4, 16, 64).  Summation order: a
 *   lane adds its elements in index order, the 64 lanes of a wave fold (6 DPP steps), the wave totals are added in wave
 *   order.  The same bits run to run.
 * dba_enc_norm: out = h(relu?(norm(x))); out == x is allowed.  stats, optional, [planes, 2] float32: (m, r) as multiplied with.
 * dba_enc_norm_skip: the tail of a residual block.  y = h(relu(norm(x))); s = skip as it is, or h(norm(d)) (the 1x1
 *   downsample branch and its norm3); out = h(relu(h(s + y))).  Exactly one of skip / d is given.  out == x is allowed.
 *   stats_d, optional and only with d: (m, r) of d's planes.
 * dba_enc_relu_skip: out = h(relu(h(skip + h(relu(x))))) over count elements (norm_fn='none'); out == x is allowed.
 * dba_enc_image: img [n, 3, H, W], src_dtype DBA_U8 or DBA_F32, BGR -> out [n, 3, H, W] of dtype, RGB:
 *   out[:, c] = ((img[:, 2 - c] * (1/255)) - mean_c) / std_c in float32, mean = (0.485, 0.456, 0.406), std = (0.229, 0.224,
 *   0.225) as float32; the product with the float32 reciprocal is what torch's `/ 255.0` runs on the device.  Rounded once
 *   to half for DBA_F16.
 * dba_enc_context_split: x [n, c_net + c_inp, hw] -> net [n, c_net, hw] = h(tanh(x[:, :c_net])) (the accurate tanhf),
 *   inp [n, c_inp, hw] = h(relu(x[:, c_net:])). */
int dba_enc_norm(const void *x, int planes, int hw, float eps, int relu, int dtype, void *out, float *stats,
                 dba_stream_t stream);
int dba_enc_norm_skip(const void *x, const void *skip, const void *d, int planes, int hw, float eps, int dtype, void *out,
                      float *stats, float *stats_d, dba_stream_t stream);
int dba_enc_relu_skip(const void *x, const void *skip, long long count, int dtype, void *out, dba_stream_t stream);
int dba_enc_image(const void *img, int n, int H, int W, int src_dtype, int dtype, void *out, dba_stream_t stream);
int dba_enc_context_split(const void *x, int n, int c_net, int c_inp, int hw, int dtype, void *net, void *inp,
                          dba_stream_t stream);

/* ---- Update operator heads (csrc/update_op.hip) ---------------------------------------------------------------------
 * The 3x3 convolutions with one or two outputs of the update operator (dbaf/droid_net.py:47-50, :91-102) with what runs
 * around them (:68, :71, :124-128), every head of a call in one launch.  All heads of a call share n, c, ht, wd and the
 * dtype, DBA_F16 or DBA_F32 (another is DBA_ERR_UNSUPPORTED); tensors are contiguous and aligned to an element.  h(.)
 * rounds to the dtype.  Per head:
 *   s   = the float32 sum over (c, ky, kx) of relu?(x)[c, y + ky - 1, x + kx - 1] * w[o, c, ky, kx], zero padding of one
 *         pixel.  SUMMATION ORDER, two levels: per pixel and output, every chunk of four channels (4 j .. 4 j + 3, the
 *         last one possibly short) has its own sum, started at +0, its terms added one by one with c ascending, within
 *         a channel ky ascending, within a row kx ascending (the order of w's memory), a padded tap as +0 * w; the chunk
 *         sums are then added one by one in chunk order to an accumulator started at +0.  Product and addition round
 *         separately (in half every product is exact in float32, only the additions round).  No atomics, no sum across
 *         lanes: the same bits run to run, on both staging routes.
 *   v   = h(s + b), b = bias[o] or 0; `sum`, when given, receives the float32 s + b that v was rounded from
 *   out = v (DBA_UPD_ACT_NONE) | h(1 / (1 + expf(-v))) (_SIGMOID) | h(scale * h(softplus(v))) (_SOFTPLUS, torch's: v > 20 ?
 *         v : log1pf(expf(v))); expf, log1pf and the division are the accurate library forms
 *   relu(x) = x > 0 ? x : (x != x ? x : 0): NaN goes through, -0 becomes +0.  GradientClip is the identity in forward.
 * out is [n, ht, wd, k]: the permute(..)[..., :k].contiguous() of the reference is the store, a pixel's two outputs as
 * one pair.  Tile: dba_upd_heads_tile's rows x cols pixels of one edge per workgroup, all channels; x is staged through LDS
 * in 16-byte vectors when hw * itemsize is a multiple of 16, every x is on a 16-byte boundary and wd <= cols, else element
 * by element.  Refused without a launch, DBA_ERR_ARG: an extent <= 0, k outside {1, 2}, n_heads outside {1, 2}, an unknown
 * act, a null x / weight / out, a pointer off its element size, a grid or n * c * ht * wd beyond 2^31 - 1, an out or sum
 * that shares a byte with any input of the call, with another head's out or sum, or with each other.  `heads` is a HOST array. */
enum { DBA_UPD_ACT_NONE = 0, DBA_UPD_ACT_SIGMOID = 1, DBA_UPD_ACT_SOFTPLUS = 2 };
typedef struct {
  const void *x;      /* [n, c, ht, wd]  the head's hidden tensor (pre-ReLU when relu_in) */
  const void *weight; /* [k, c, 3, 3]    same dtype as x */
  const void *bias;   /* [k] or NULL */
  void *out;          /* [n, ht, wd, k]  same dtype */
  float *sum;         /* optional [n, ht, wd, k] float32: s + b as it was rounded from */
  int k;              /* 1 or 2 */
  int relu_in;        /* apply ReLU to x as it is read */
  int act;            /* DBA_UPD_ACT_NONE | _SIGMOID | _SOFTPLUS */
  float scale;        /* _SOFTPLUS only: out = h(scale * h(softplus(v))) */
  int out_f32;        /* != 0: out is float32 [n, ht, wd, k] whatever the dtype (autocast's softplus answers so): v = h(s + b)
                         as before, then the activation in float32 with NO rounding behind it: v | 1 / (1 + expf(-v)) |
                         scale * softplus(v) */
} dba_upd_head_t;
int dba_upd_heads(const dba_upd_head_t *heads, int n_heads, int n, int c, int ht, int wd, int dtype, dba_stream_t stream);
int dba_upd_heads_tile(int *rows, int *cols); /* the kernel's tile extents, for the tests */

/* ---- map export (csrc/map_export.hip) ---------------------------------------------------------------------------------
 * The keyframe archive of DepthVideo.ba (dbaf/depth_video.py:337-343, :379-385) and the point cloud of save_vis_easy
 * (dbaf/dbaf.py:64-140).  All pointers are device pointers unless named otherwise; nothing is read back by the library.
 *
 * dba_archive_frames: ONE launch.  Frames [i0, i1) of the video buffers go to rows [row, row + i1 - i0) of the save buffers:
 *   tstamp (double), disps [.., ht, wd], poses [.., 7] and, when disps_up / disps_up_save are not null, disps_up (rows of
 *   up_elems floats) are row copies; images_save[r, y, x, c] = float(images[i, 2 - c, 8 y, 8 x]) * (1.0f / 255.0f), the bits
 *   torch writes for `images[i, [2,1,0], ::8, ::8].permute(1,2,0) / 255.0` on device tensors (it multiplies by the float32
 *   reciprocal of a host scalar).  images is uint8 [n_src, 3, img_h, img_w]; needs ht == ceil(img_h / 8), wd == ceil(img_w / 8),
 *   0 <= i0, i1 <= n_src, 0 <= row, row + (i1 - i0) <= n_dst, i1 - i0 <= 65535.  i1 <= i0: no launch.
 * dba_map_plan: per archived frame b < count: means[b] (float32 mean of disps_save[b]: lane l of 256 adds pixels l, l + 256,
 *   ...; a wave tree; the four wave totals in wave order; one IEEE division), inv_poses[b] (SE3(pose).inv(), 7 floats) and
 *   cameras[b] (its 4x4 matrix, row-major).  scalars[0] = the lower median of the means (torch.median), scalars[1] = the
 *   threshold: ((0.4f * 1.0f) / 4.0f) * (1.0f / median) when min_count > 0 (filtered), 0.4f otherwise (raw, unused).
 *   counts [count, ht, wd] (filtered only): the depth-filter count with neighbours over ALL `rows` rows of the save buffers;
 *   mask [count, ht, wd] (bytes 0 / 1): (counts >= min_count) & (disp > 0.5f * means[b]), raw: the second clause alone, and no
 *   depth-filter code runs; frame_counts [count] (int): survivors per frame; offsets [count + 1]: their exclusive scan,
 *   offsets[count] the total.  tickets: two ints, ZERO on entry.  *launches (host): the launches enqueued, 2 filtered, 1 raw.
 *   Needs 0 <= count <= rows, ht, wd >= 1; the save buffers have `rows` rows.  count == 0: no launch.
 * dba_map_payload: ONE launch.  pts [total, 3] = the points of the surviving pixels (iproj on inv_poses), clr [total, 3] their
 *   rows of images_save [rows, ht, wd, 3], frame-major and row-major within a frame; total == offsets[count] as the host
 *   read it.  total == 0: no launch. */
int dba_archive_frames(const double *tstamp, const float *disps, const float *poses, const float *disps_up,
                       const uint8_t *images, double *tstamp_save, float *disps_save, float *poses_save,
                       float *disps_up_save, float *images_save, int n_src, int n_dst, int i0, int i1, int row, int ht,
                       int wd, int img_h, int img_w, int64_t up_elems, dba_stream_t stream);
int dba_map_plan(const float *poses_save, const float *disps_save, const float *intrinsics, int count, int rows, int ht,
                 int wd, int min_count, float *means, float *inv_poses, float *cameras, float *scalars, float *counts,
                 uint8_t *mask, int *frame_counts, int64_t *offsets, int *tickets, int *launches, dba_stream_t stream);
int dba_map_payload(const float *inv_poses, const float *disps_save, const float *intrinsics, const float *images_save,
                    const uint8_t *mask, const int64_t *offsets, int count, int rows, int ht, int wd, int64_t total,
                    float *pts, float *clr, dba_stream_t stream);

/* ---- frame admission (csrc/frames.hip) --------------------------------------------------------------------------------
 * How a frame enters and leaves the window: DepthVideo.append (dbaf/depth_video.py:129-159, :183-185), the seeds for the
 * next frame (dbaf/dbaf_frontend.py:372-375, :841-849) and the pose hand-over with the host estimator (:224-228, :424-432,
 * :553-570, :607-608, :809-814).  Device pointers unless named host.
 *
 * dba_frame_append: ONE launch that writes row `row` of the video buffers from a dba_frame_item (read on the host).
 *   tstamp[row] = tstamp_value.  image / fmap / net / inp (null: the row is left alone) are dense rows moved by the row
 *   mover's job table (csrc/row_jobs.h), rows of 3 * 64 ht wd, fmap_row_bytes, net_row_bytes, inp_row_bytes bytes; they must
 *   not overlap the rows they are written to.  pose (7 floats) and intr (4 floats): DBA_FR_SKIP, DBA_FR_HOST (the values of
 *   the struct, carried in the kernel's arguments) or DBA_FR_DEVICE (pose_dev / intr_dev are read by the launch).  disp:
 *   DBA_FR_SKIP, DBA_FR_HOST (every entry of disps[row] = disp_fill) or DBA_FR_DEVICE (disp_dev, [ht, wd]).  depth (null, or
 *   [8 ht, 8 wd] floats): disps_sens[row][y, x] = d > 0 ? 1 / d : d with d = depth[8 y + 3, 8 x + 3], one IEEE division.
 *   seed_disps != 0: afterwards disps[row] = disps_sens[row] > 0 ? disps_sens[row] : disps[row] (dbaf_frontend.py:247-248),
 *   on the values this call leaves in both rows.  Needs 0 <= row < rows, ht, wd >= 1.
 * dba_frame_seed_next: ONE launch of one workgroup.  poses[t1] = poses[t1 - 1]; every entry of disps[t1] = the float32 mean
 *   of disps[t1 - mean_rows : t1] in one fixed order (csrc/frames.hip); dirty[lo : t1] = 1 with lo = min(ii) clamped to
 *   [0, t1], lo = 0 when ii is null.  Needs 1 <= mean_rows <= t1 < rows, t1 <= dirty_rows, mean_rows * ht * wd <= 2^24,
 *   n_ii >= 1 when ii is not null.
 * dba_world_poses: out_host[r] (16 floats, row-major) = SE3(poses[r]).inv().matrix() for r < n, by the routine of
 *   dba_keyframe_check.  ONE launch into pinned memory of the library's, one host wait on a completion word (no stream
 *   synchronisation), then a host copy into out_host.  Needs 1 <= n <= rows, n <= DBA_FR_MAX_ROWS.
 * dba_set_world_poses: wTc_host: n row-major 4x4 doubles, camera-to-world, for rows [i0, i0 + n).  ONE launch: in float64,
 *   world-to-camera as (R^T, -R^T t), the quaternion by the four-branch rule (the largest of the diagonal entries and the
 *   trace picks the branch, the first on a tie; no sign canonicalisation), normalised, rounded to float32 into poses[i].
 *   inv_scale != 0: disps[i] *= inv_scale on the same rows.  The matrices are staged through pinned memory of the library's:
 *   wTc_host is free on return.  Nothing synchronises the stream; a completion word guards the staging block's reuse, and
 *   *waited (host, may be null) says whether this call had to wait for it.  Needs 0 <= i0, i0 + n <= rows, 1 <= n <=
 *   DBA_FR_MAX_ROWS, disps_rows >= i0 + n when inv_scale != 0. */
#define DBA_FR_SKIP 0
#define DBA_FR_HOST 1
#define DBA_FR_DEVICE 2
#define DBA_FR_MAX_ROWS 1024
typedef struct dba_frame_item {
  void *tstamp, *images, *poses, *disps, *disps_sens, *intrinsics, *fmaps, *nets, *inps; /* the video's buffers */
  int rows, row, ht, wd;
  int64_t fmap_row_bytes, net_row_bytes, inp_row_bytes;
  double tstamp_value;
  const void *image, *fmap, *net, *inp;
  const float *pose_dev, *intr_dev, *disp_dev, *depth;
  int pose_mode, intr_mode, disp_mode, seed_disps;
  float pose[7], intr[4], disp_fill;
} dba_frame_item;
int dba_frame_append(const dba_frame_item *item_host, dba_stream_t stream);
int dba_frame_seed_next(float *poses, float *disps, uint8_t *dirty, int rows, int dirty_rows, int ht, int wd, int t1,
                        int mean_rows, const int64_t *ii, int64_t n_ii, dba_stream_t stream);
int dba_world_poses(const float *poses, int rows, int n, float *out_host, dba_stream_t stream);
int dba_set_world_poses(float *poses, float *disps, int rows, int disps_rows, int64_t map_elems, int i0, int n,
                        const double *wTc_host, float inv_scale, int *waited, dba_stream_t stream);

#define DBA_PEER_TIMEOUT 1
size_t dba_peer_exchange_bytes(size_t max_doubles);
int dba_peer_exchange_create(size_t bytes, void **region, unsigned char *handle64);
int dba_peer_exchange_open(const unsigned char *handle64, void **region);
int dba_peer_exchange_close(void *region, int opened);
int dba_peer_allreduce_f64(double *buf, size_t n, void *const *regions, int rank, int world, unsigned epoch,
                           size_t max_doubles, int *status, dba_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DBA_HIP_H */
