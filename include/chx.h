/* chx.h — C-ABI of libchx, the MI355X (gfx950) beam-dynamics tracking engine.
 *
 * This is the drop-in boundary of the `Segment.track(ParticleBeam)` hot path of
 * desy-ml/cheetah. The reference has no FFI of its own (it is pure Python on
 * PyTorch); its operator interface is `Element.track` /
 * `Element.first_order_transfer_map` / `Segment.track` / `ParticleBeam`
 * (cheetah/accelerator/element.py:104-193, cheetah/accelerator/segment.py:534-574,
 * cheetah/particles/particle_beam.py:60-106). Every entry point below names the
 * reference function (file:line under /root/reference/cheetah) whose arithmetic it
 * replaces. `cheetah_amd/_lib.py` binds them with ctypes; INTEGRATION.md shows the
 * stub a Cheetah maintainer would add.
 *
 * Conventions (all entry points)
 *  - return CHX_OK (0) or a negative chx_status; nothing throws across the ABI;
 *  - every pointer is a DEVICE pointer owned by the caller, except `const int32_t*`
 *    / struct arguments which are HOST memory read before the call returns;
 *  - no allocation, no host synchronisation, no global state: work is enqueued on
 *    the caller's HIP stream (`stream` = hipStream_t, NULL = default stream) and the
 *    call returns immediately; calls on different streams are re-entrant;
 *  - dtype: CHX_F32 / CHX_F64 selects the element type of all `void*` floating
 *    buffers of that call; `double*` buffers are always fp64;
 *  - phase-space layout is the reference's: particles[B][N][7] row-major, row =
 *    (x, px, y, py, tau, delta, 1) (element.py:104-131), transfer maps [B][7][7]
 *    row-major with out_i = sum_j R[i][j] * in_j (element.py:182);
 *  - "B?" arguments (Bx, BR, Bw, ...) are broadcast extents: each must be 1 or B.
 *  - particle buffers must be 16-byte aligned (CHX_ERR_MISALIGNED otherwise).
 */
#ifndef CHX_H
#define CHX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHX_ABI_VERSION 9 /* 2: ldz argument of chx_sc_igf / chx_sc_gradient; 3: post_map arguments of chx_sc_kick;
                             4: s_in / s_out arguments of chx_run_map / chx_run_track;
                             5: s_in / s_out arguments of chx_cavity_prepare_scalars / chx_cavity_track_scalars;
                             6: chx_lattice_track_diag (items of type 2 / 3 in the table of a lattice stretch);
                             7: chx_lattice_track_screens / chx_parameter_lattice_track_screens (items of type 4: active Screens);
                             8: chx_lattice_screen.mom_partials, chx_table_store; 9: chx_run_vjp_entry */

typedef enum chx_status {
    CHX_OK = 0,
    CHX_ERR_INVALID_ARG = -1,
    CHX_ERR_DTYPE = -2,
    CHX_ERR_MISALIGNED = -3,
    CHX_ERR_LAUNCH = -4,
    CHX_ERR_WORKSPACE = -5,
    CHX_ERR_NO_DEVICE = -6
} chx_status;

typedef enum chx_dtype { CHX_F32 = 0, CHX_F64 = 1 } chx_dtype;

/* Element kinds understood by chx_build_rmatrix; params layout [P] per batch row. */
typedef enum chx_kind {
    CHX_IDENTITY = 0,   /* P=0  Marker / inactive Screen, BPM, Aperture (marker.py:45-57) */
    CHX_DRIFT = 1,      /* P=1  [L]                                  track_methods.py:284-299 */
    CHX_QUADRUPOLE = 2, /* P=5  [L,k1,tilt,mis_x,mis_y]              quadrupole.py:93-110     */
    CHX_DIPOLE = 3,     /* P=9  [L,angle,k1,e1,e2,tilt,fint,fint_exit,gap]  dipole.py:372-394,430-466 */
    CHX_HCOR = 4,       /* P=2  [L,angle]                            horizontal_corrector.py:60-78 */
    CHX_VCOR = 5,       /* P=2  [L,angle]                            vertical_corrector.py:61-78 */
    CHX_CCOR = 6,       /* P=3  [L,hangle,vangle]                    combined_corrector.py:77-98 */
    CHX_CAVITY_SW = 7,  /* P=4  [L,voltage,phase_deg,frequency]      cavity.py:253-358 (standing wave) */
    CHX_CAVITY_TW = 8,  /* P=4  same, traveling wave                 cavity.py:310-335 */
    CHX_SOLENOID = 9,   /* P=4  [L,k,mis_x,mis_y]                    solenoid.py:75-116  (row f3) */
    CHX_UNDULATOR = 10, /* P=4  [L,kx,ky,period]                     undulator.py:79-125 (row f3) */
    CHX_KIND_COUNT = 11
} chx_kind;

#define CHX_MAX_PARAMS 9
/* number of params of a kind, or -1 */
int chx_kind_num_params(int kind);
int chx_abi_version(void);
/* human-readable status */
const char* chx_status_string(int status);

/* ---- map builders (a3-a8; track_methods.py:17-77,284-382; dipole.py:430-466; cavity.py:253-358)
 * Builds R_out[B][7][7] (dtype) from params[Bp][P] and energy[Be] (dtype). Arithmetic is
 * carried out in fp64 on device and rounded once. mass_eV / n_charges describe the Species
 * (species.py:30-36). */
int chx_build_rmatrix(int kind, const void* params, const void* energy, double mass_eV,
                      double n_charges, int64_t B, int64_t Bp, int64_t Be, int dtype,
                      void* R_out, void* stream);

/* Vector-Jacobian product of chx_build_rmatrix: given dR[B][7][7] (dtype) returns
 * dparams[B][P] and denergy[B] (dtype), d(sum dR*R)/d(param). Forward-mode dual numbers
 * inside the kernel; replaces autograd through track_methods.py / utils/autograd.py:77-146. */
int chx_build_rmatrix_vjp(int kind, const void* params, const void* energy, double mass_eV,
                          double n_charges, const void* dR, int64_t B, int64_t Bp, int64_t Be,
                          int dtype, void* dparams, void* denergy, void* stream);

/* Maps of E elements whose parameters are SCALARS, read where they live: kinds[E] and param_ptrs[E][CHX_MAX_PARAMS]
 * (host arrays; entry k of element e is a DEVICE pointer to one `dtype` value, in the order chx_build_rmatrix documents;
 * unused entries NULL), energy = device pointer to one value -> R_out[E][7][7]. Same arithmetic and rounding as E calls
 * of chx_build_rmatrix with B = 1; made for control loops that change a few settings and re-track (one call instead of a
 * packed tensor, an allocation and a launch per element). */
int chx_build_rmatrix_scalars(const int32_t* kinds, const void* const* param_ptrs, int64_t E, const void* energy,
                              double mass_eV, double n_charges, int dtype, void* R_out, void* stream);
/* Persistent map of a run of scalar-parameter elements (Segment.track's steady state, segment.py:545-574): `state`
 * (chx_run_state_bytes(E) bytes of device memory owned by the caller, filled with 0xFF bytes once) remembers the parameter
 * values, the element maps and the composed map R of the last call. chx_run_map launches ONE workgroup that re-reads every
 * parameter through its pointer and returns at once if none changed, else rebuilds and recomposes — bit-identical to
 * chx_build_rmatrix_scalars + chx_compose_maps. *R_out (if not NULL) receives the device address of R[7][7] inside `state`.
 * chx_run_track = chx_run_map + chx_apply_affine7(x_in, R, x_out) for one beam of N particles: a whole merged
 * Segment.track in one call, with no host-side validation of the settings. E <= 192 elements, <= 400 parameters in total
 * (CHX_ERR_INVALID_ARG beyond: use the two-call form). Identity elements are left out by the caller.
 * s_in / s_out (both NULL or both device pointers to one `dtype` value): the path length behind the run,
 * *s_out = *s_in + (((L_0 + L_1) + L_2) + ...) with the lengths read from the settings on every call (the first parameter of
 * every kind), like `incoming.s + segment.length` (segment.py:54-58): no host copy that an edited length could leave stale. */
/* Prefix products of a run: out[e][b] = maps[e][b] ... maps[1][b] maps[0][b] for every e (maps[E][Bm][7][7], Bm in {1, B};
 * out[E][B][7][7]); fp64 accumulation carried along, each prefix rounded once. With chx_track_moments on the E prefixes the
 * beam moments after every element of a lattice (segment.py:658-700 `get_beam_attrs_along_segment`) cost one pass over the
 * particles instead of E tracking passes and E reductions. */
int chx_compose_prefix(const void* maps, int64_t E, int64_t B, int64_t Bm, int dtype, void* out, void* stream);
/* Backward of chx_build_rmatrix_scalars + chx_compose_maps for a run whose settings carry gradients (autograd through
 * segment.py:534-574 for scalar parameters): given the element maps maps[E][7][7] of the forward call and dT[7][7] =
 * dL/d(composed map) (both `dtype`), writes dinputs[E][CHX_MAX_PARAMS + 1] (`dtype`): column k < P_e is dL/d(parameter k of
 * element e), column CHX_MAX_PARAMS is element e's contribution to dL/d(energy), the other columns are zero. Two launches
 * (a one-wave prefix / suffix sweep in fp64, then dual-number builders), workspace chx_run_vjp_workspace_bytes(E). */
size_t chx_run_vjp_workspace_bytes(int64_t E);
int chx_run_vjp(const int32_t* kinds, const void* const* param_ptrs, int64_t E, const void* energy, double mass_eV,
                double n_charges, int dtype, const void* maps, const void* dT, void* dinputs, void* workspace,
                size_t workspace_bytes, void* stream);
/* The same with a mask: need[E] (NULL = everything), bit k of need[e] set = slot k of element e is wanted (bit
 * CHX_MAX_PARAMS: the energy); unwanted slots are written as zeros without evaluating their dual-number builder (a loss on
 * ONE quadrupole strength of a 100-element run evaluates one builder, not 250). */
int chx_run_vjp_masked(const int32_t* kinds, const void* const* param_ptrs, int64_t E, const void* energy, double mass_eV,
                       double n_charges, int dtype, const void* maps, const void* dT, const uint16_t* need, void* dinputs,
                       void* workspace, size_t workspace_bytes, void* stream);
/* ABI 9. The same when dL/d(composed map) comes from ONE property of the beam y = C x the run's map produced — entry `index` (2..28)
 * of chx_moments(y) = mom_y[29], or its square root (`take_sqrt`), with the gradient grad[1] (`dtype`) — instead of a tensor dT:
 * every wave of the builders' launch forms chx_moment_entry_mapped_bwd's 49 values itself (C[7][7] `dtype`: the composed map,
 * mom_x[29]: the incoming beam's moments), rounded to `dtype` as that call writes them. The backward pass of
 * d sigma_x(screen) / d k1 (tests/test_differentiable.py:10-32; screen.py:187-239, particle_beam.py:1672-1943) is then ONE launch.
 * Runs of more than 16 elements fall back to the two launches. Workspace: chx_run_vjp_entry_workspace_bytes(E). */
size_t chx_run_vjp_entry_workspace_bytes(int64_t E);
int chx_run_vjp_entry(const int32_t* kinds, const void* const* param_ptrs, int64_t E, const void* energy, double mass_eV,
                      double n_charges, int dtype, const void* maps, const uint16_t* need, const void* grad, const double* mom_y,
                      int index, int take_sqrt, const void* C, const double* mom_x, void* dinputs, void* workspace,
                      size_t workspace_bytes, void* stream);
/* A merged run whose settings are VECTORISED over B lattice settings (segment.py:534-547 with (B,) parameters: a k1 scan, a batched
 * environment, an orbit response): all B composed maps R_out[B][7][7] in one launch — per row the element maps of chx_build_rmatrix
 * and the product of chx_compose_maps, bit-identical to those calls. batched[E][CHX_MAX_PARAMS]: 1 = the pointer addresses a
 * contiguous (B,) array of `dtype`, 0 = a scalar; every length (parameter 0) is a scalar; energy_rows != 0: `energy` is a (B,)
 * array as well (a scan of beam energies, with or without vectorised settings), else a scalar.
 * workspace: chx_run_map_batched_workspace_bytes(E, B, dtype) bytes (0 when a row's element maps fit the LDS). */
size_t chx_run_map_batched_workspace_bytes(int64_t E, int64_t B, int dtype);
int chx_run_map_batched(const int32_t* kinds, const void* const* param_ptrs, const uint8_t* batched, int64_t E, int64_t B,
                        const void* energy, int energy_rows, double mass_eV, double n_charges, int dtype, void* workspace,
                        size_t workspace_bytes, void* R_out, void* stream);
/* Forward of the same run in one call: chx_build_rmatrix_scalars into maps[E][7][7] (kept for chx_run_vjp) followed by
 * chx_compose_maps of that stack into R_out[7][7]; bit-identical to the two calls (segment.py:534-543). E <= 4096. */
int chx_run_build_compose(const int32_t* kinds, const void* const* param_ptrs, int64_t E, const void* energy, double mass_eV,
                          double n_charges, int dtype, void* maps, void* R_out, void* stream);
size_t chx_run_state_bytes(int64_t E);
int chx_run_map(const int32_t* kinds, const void* const* param_ptrs, int64_t E, const void* energy, double mass_eV,
                double n_charges, int dtype, void* state, size_t state_bytes, void** R_out, const void* s_in, void* s_out,
                void* stream);
int chx_run_track(const int32_t* kinds, const void* const* param_ptrs, int64_t E, const void* energy, double mass_eV,
                  double n_charges, int dtype, void* state, size_t state_bytes, const void* x_in, void* x_out, int64_t N,
                  const void* s_in, void* s_out, void* stream);
/* ---- segment composition (a2; segment.py:534-543): R_out[b] = R_{E-1}[b] ... R_1[b] R_0[b].
 * R_ptrs is a HOST array of E device pointers, one map buffer per element (each element owns
 * its cached map); buffer e is [1][7][7] if bcast[e] (HOST array) else [B][7][7]. The pointers are
 * forwarded by value in the kernel arguments (no device-side table, no copy). fp64 accumulation,
 * rounded once to dtype. */
int chx_compose_maps(const void* const* R_ptrs, const uint8_t* bcast, int64_t E, int64_t B,
                     int dtype, void* R_out, void* stream);
/* Backward of chx_compose_maps (autograd through segment.py:534-543 for vectorised maps): given dT[B][7][7] = dL/d(composed map)
 * writes dM[E][B][7][7] = dL/d(element map e of batch row b) (dtype; the caller sums the rows of a broadcast map). One wave per
 * batch row, fp64 prefix / suffix sweep. E <= 192; workspace chx_compose_maps_vjp_workspace_bytes(E, B). */
size_t chx_compose_maps_vjp_workspace_bytes(int64_t E, int64_t B);
int chx_compose_maps_vjp(const void* const* R_ptrs, const uint8_t* bcast, int64_t E, int64_t B, int dtype, const void* dT, void* dM,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- linear apply (a1; element.py:180-191): x_out[b][n][:] = R[b] . x_in[b][n][:]. */
int chx_apply_affine7(const void* x_in, const void* R, void* x_out, int64_t B, int64_t Bx,
                      int64_t BR, int64_t N, int dtype, void* stream);

/* Backward of the apply: dX[b][n][j] = sum_i dY[b][n][i] R[b][i][j]  (dX may be NULL) and
 * dR[b][i][j] = sum_n dY[b][n][i] X[b][n][j] (double dR[B][49]; may be NULL; needs workspace
 * of chx_apply_bwd_workspace_bytes(B,N)). */
size_t chx_apply_bwd_workspace_bytes(int64_t B, int64_t N);
int chx_apply_affine7_bwd(const void* dY, const void* R, const void* X, void* dX, double* dR,
                          int64_t B, int64_t Bx, int64_t BR, int64_t N, int dtype,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Element-by-element tracking of a run of E linear elements WITHOUT merging the maps
 * (`for e in elements: beam = e.track(beam)`, segment.py:571-572): E apply passes
 * pass 0 writes x_out, later passes update x_out in place (tile-local read-then-write). x_out must not alias x_in, which is
 * only read.
 * `scratch`: NULL, or at least chx_track_elementwise_scratch_bytes(B, N, dtype) bytes of device memory (4-byte aligned; the
 * function returns 0 where no call of these extents uses scratch, and then any pointer is ignored). It needs no initialising
 * and holds nothing of use after the call: one word per tile of the column layout below, in which the pass that enters the
 * layout records that the tile's seventh coordinate is 1 in every row — true of every beam this library makes, and kept so by
 * every map whose last row is (0,...,0,1) — so that the passes in between do not read that column; a pass whose map makes it
 * anything else stores the column and withdraws the word. The results are bit for bit those of a call with scratch == NULL,
 * whatever the beam and the maps hold.
 * (An additive export: CHX_ABI_VERSION stays as it is, as for every function added without changing an existing one.)
 * With E >= 3, 16-byte aligned batch rows and 8 MiB of particles or more, the full tiles of x_out (512 float32 / 256 float64
 * rows) are held transposed, [7][rows], between pass 1 and pass E-1, and a pass in between stores only the coordinates whose
 * bits its map changed. Pass E-1 writes rows again: x_out holds [B][N][7] rows, bit for bit those of E plain passes, once the
 * call's last kernel has run (stream order, as for any output); it must not be read on another stream before that. */
size_t chx_track_elementwise_scratch_bytes(int64_t B, int64_t N, int dtype);
int chx_track_elementwise(const void* x_in, const void* R /*[E][BR][7][7]*/, void* x_out,
                          void* scratch, int64_t E, int64_t B, int64_t Bx, int64_t BR,
                          int64_t N, int dtype, void* stream);

/* Same result as chx_track_elementwise (bit-identical per-element rounding) but one pass
 * over HBM: each particle stays in registers while the E maps are applied in order. */
int chx_track_fused(const void* x_in, const void* R /*[E][BR][7][7]*/, void* x_out, int64_t E,
                    int64_t B, int64_t Bx, int64_t BR, int64_t N, int dtype, void* stream);

/* ---- cavity (a8; cavity.py:100-251).
 * coefficients per batch row, computed on device (no host branch: the reference's
 * `if (delta_energy > 0).any()` (cavity.py:157) is evaluated over the batch in-kernel). */
#define CHX_CAV_NCOEF 8 /* [a, b, kbeta0, phi, cosphi, T566, T556, T555] */
int chx_cavity_coeffs(const void* params /*[Bp][4]*/, const void* energy /*[Be]*/, double mass_eV,
                      double n_charges, int64_t B, int64_t Bp, int64_t Be, int dtype,
                      double* coeffs /*[B][CHX_CAV_NCOEF]*/, void* energy_out /*[B] dtype*/,
                      void* stream);
/* x_out = R.x_in, then delta' and tau' per particle (cavity.py:135-151,220-226). */
int chx_cavity_track(const void* x_in, const void* R, const double* coeffs, void* x_out,
                     int64_t B, int64_t Bx, int64_t N, int dtype, void* stream);

/* Backward of the per-particle part of chx_cavity_track that is not the matrix apply: given dY = dL/d(x_out), adds
 * the delta' / tau' rewrite's contribution to dX[B][N][7] (columns tau, delta; dX may be NULL) and writes
 * dcoeffs[B][CHX_CAV_NCOEF] = dL/d(coeffs). The matrix part is chx_apply_affine7_bwd with row 5 of R zeroed.
 * workspace: chx_moments_workspace_bytes(B, N). */
int chx_cavity_track_bwd(const void* dY, const void* X, const double* coeffs, void* dX, double* dcoeffs, int64_t B,
                         int64_t Bx, int64_t N, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---- weighted beam moments (a10; particle_beam.py:1672-1943, utils/statistics.py:4-62).
 * sums[b] = { W=sum w, sum w^2, sum w x_0..5 }  (8 doubles)
 * m2[b]   = upper triangle (a<=b, row-major, 21 doubles) of sum w (x_a-mu_a)(x_b-mu_b),
 *           mu = sums[2..7]/sums[0] read from `sums` on device (multi-GPU: all-reduce sums first)
 * out[b]  = { W, W2, mu[6], cov[21] } with cov = m2 / (W - W2/W)          (29 doubles)
 * w may be NULL (all ones). Deterministic two-stage reductions (no float atomics). */
#define CHX_MOM_NSUMS 8
#define CHX_MOM_NM2 21
#define CHX_MOM_NOUT 29
size_t chx_moments_workspace_bytes(int64_t B, int64_t N);
int chx_moment_sums(const void* x, const void* w, int64_t B, int64_t Bx, int64_t Bw, int64_t N,
                    int dtype, double* sums, void* workspace, size_t workspace_bytes, void* stream);
int chx_moment_centred(const void* x, const void* w, const double* sums, int64_t B, int64_t Bx,
                       int64_t Bw, int64_t N, int dtype, double* m2, void* workspace,
                       size_t workspace_bytes, void* stream);
int chx_moment_finalize(const double* sums, const double* m2, int64_t B, double* out, void* stream);
/* convenience: the three calls above on one stream */
int chx_moments(const void* x, const void* w, int64_t B, int64_t Bx, int64_t Bw, int64_t N,
                int dtype, double* out, void* workspace, size_t workspace_bytes, void* stream);
/* chx_moments plus ONE entry of the vector in the beam dtype — what a beam property reads (particle_beam.py:1672-1943: mu_*,
 * sigma_* = sqrt of the variance, cov_*): entry_out[B] (dtype) = out[b][index] or its square root, written by the same finalize
 * launch (index < 0: plain chx_moments). */
int chx_moments_entry(const void* x, const void* w, int64_t B, int64_t Bx, int64_t Bw, int64_t N, int dtype, double* out,
                      int index, int take_sqrt, void* entry_out, void* workspace, size_t workspace_bytes, void* stream);
/* Multi-GPU: exact merge of the chx_moments outputs of R particle shards, per_rank[R][B][29] -> out[B][29] (the reference's
 * weighted statistics over the union of the shards, utils/statistics.py:30-48; shards with zero weight are skipped). */
int chx_merge_moments(const double* per_rank, int32_t R, int64_t B, double* out, void* stream);
/* backward of chx_moments wrt x: given d_out[B][29] (double; entries 0,1 ignored) */
int chx_moments_bwd(const void* x, const void* w, const double* out, const double* d_out,
                    int64_t B, int64_t Bx, int64_t Bw, int64_t N, int dtype, void* dX, void* stream);
/* The same with the gradient of the WEIGHTS as well (utils/statistics.py:4-62 is differentiable in the survival
 * probabilities: an Aperture with trainable edges upstream): dW[B][N] (dtype; the caller sums the rows of a broadcast weight
 * array), dX and dW may each be NULL. d_out entries 0 (W) and 1 (sum w^2) are honoured here. */
int chx_moments_bwd_w(const void* x, const void* w, const double* out, const double* d_out, int64_t B, int64_t Bx, int64_t Bw,
                      int64_t N, int dtype, void* dX, void* dW, void* stream);
/* ---- slice statistics (ParticleBeam.slice_statistics): the particles of row b whose tau (column 4) falls into slice k of
 * edges[Be][S + 1] (dtype, increasing; torch.histogram's membership: tau < e_0, tau > e_S and NaN are in no slice, tau == e_S is
 * in the last one) -> out[B][S][29] with chx_moments' statistics of those particles alone (slices without weight: its NaN
 * pattern) and charge[B][S] = sum q w. w, q (dtype, [Bw][N], [Bq][N]) may be NULL (all ones). 1 <= S <= CHX_SLICES_MAX.
 * Deterministic: a stable counting sort by slice, fixed pieces of every slice reduced in fp64 about their own mean, the pieces
 * merged in order; no float atomics. workspace: chx_slice_moments_workspace_bytes(B, N, S) (also for the backward pass).
 * chx_slice_moments_bwd: given d_out[B][S][29] and d_charge[B][S] (either may be NULL) -> dX[B][N][7], dW[B][N], dQ[B][N]
 * (dtype; NULL outputs are not computed; rows of broadcast inputs are NOT reduced — the caller sums). A particle in slice k gets
 * chx_moments_bwd_w's gradient with row k of out / d_out plus the charge terms; particles in no slice and slices whose
 * cotangent is zero contribute exactly 0. */
#define CHX_SLICES_MAX 2048
size_t chx_slice_moments_workspace_bytes(int64_t B, int64_t N, int32_t S);
int chx_slice_moments(const void* x, const void* w, const void* q, const void* edges, int64_t B, int64_t Bx, int64_t Bw, int64_t Bq,
                      int64_t Be, int64_t N, int32_t S, int dtype, double* out, double* charge, void* workspace,
                      size_t workspace_bytes, void* stream);
int chx_slice_moments_bwd(const void* x, const void* w, const void* q, const void* edges, int64_t B, int64_t Bx, int64_t Bw,
                          int64_t Bq, int64_t Be, int64_t N, int32_t S, int dtype, const double* out, const double* d_out,
                          const double* d_charge, void* dX, void* dW, void* dQ, void* workspace, size_t workspace_bytes,
                          void* stream);
/* ---- bunching factor (ParticleBeam.bunching_factor): per batch row b and spatial frequency nu[Bnu][K] (fp64, TURNS per metre:
 * nu = 1 / lambda = k / (2 pi), so that no rounding of 2 pi enters the phase), with a_i = q_i w_i and tau column 4 of x:
 *   F[B][K][2] = sum_i a_i exp(-2 pi i nu tau_i) (re, im),  Q[B] = sum_i a_i      (the bunching factor is F / Q)
 * The phase is t = nu * tau in fp64, reduced to f = t - rint(t); sin and cos of 2 pi f are evaluated in the beam's precision
 * (dtype) and accumulated in fp64. A particle with a == 0 contributes exactly 0 whatever its tau holds (a select, not a
 * product: lost particles keep NaN / inf coordinates); a non-finite tau with a != 0 makes every F of its row NaN.
 * w, q (dtype, [Bw][N], [Bq][N]) may be NULL (all ones). 1 <= K <= CHX_BUNCHING_K_MAX.
 * Deterministic: a direct sum over CHX_BUNCHING_CHUNK particles x CHX_BUNCHING_K_TILE frequencies per workgroup, every
 * frequency one fma chain per wave, the waves and then the chunks added in a fixed order; no float atomics.
 * workspace: chx_bunching_workspace_bytes(B, N, K) (0 for arguments out of range); the backward pass needs none (its workspace
 * arguments are accepted and ignored).
 * chx_bunching_bwd: given dF[B][K][2] and dQ[B] (either may be NULL) -> dTau[B][N], dW[B][N], dQpart[B][N] (dtype; NULL outputs
 * are not computed; rows of broadcast inputs are NOT reduced — the caller sums). With theta = 2 pi nu_k tau_i:
 *   dTau_i = a_i sum_k 2 pi nu_k (-dF_re sin theta - dF_im cos theta),  da_i = sum_k (dF_re cos theta - dF_im sin theta) + dQ,
 *   dQpart_i = da_i w_i,  dW_i = da_i q_i.
 * A particle with a == 0 gets dTau == 0 exactly; if its tau is not finite as well, the sum over k in da_i is taken as 0. */
#define CHX_BUNCHING_K_MAX 65536  /* 256 frequency tiles (a grid dimension); F partials: 16 K bytes per chunk and row */
#define CHX_BUNCHING_CHUNK 2048   /* particles per workgroup: the granule of the ordered merge */
#define CHX_BUNCHING_K_TILE 256   /* frequencies per workgroup */
size_t chx_bunching_workspace_bytes(int64_t B, int64_t N, int64_t K);
int chx_bunching(const void* x, const void* w, const void* q, const double* nu, int64_t B, int64_t Bx, int64_t Bw, int64_t Bq,
                 int64_t Bnu, int64_t N, int64_t K, int dtype, double* F, double* Q, void* workspace, size_t workspace_bytes,
                 void* stream);
int chx_bunching_bwd(const void* x, const void* w, const void* q, const double* nu, int64_t B, int64_t Bx, int64_t Bw, int64_t Bq,
                     int64_t Bnu, int64_t N, int64_t K, int dtype, const double* dF, const double* dQ, void* dTau, void* dW,
                     void* dQpart, void* workspace, size_t workspace_bytes, void* stream);
/* ---- tunes from turn-by-turn records (TurnByTurn.tunes): probe[R][S][7] (dtype) holds S rows at R consecutive records. One
 * signal is column c = 0 (x), 2 (y) or 4 (tau) of one row over the records r0 .. r0 + T - 1: u_n, n < T, exactly as float64. With
 * the Hann window w_n = sin^2(pi (n + 1/2) / T), the windowed mean m = sum w u / sum w and v_n = w_n (u_n - m), all in float64:
 *   F(nu) = sum v_n exp(-2 pi i nu n), G(nu) = sum n v_n exp(-2 pi i nu n), A = |F|^2, dA / dnu = 4 pi g, g = F_r G_i - F_i G_r,
 * the phase nu n reduced in turns (its fractional part) before sin / cos. Coarse grid nu_k = k / (2 P), k = 0 .. P, with
 * P = 2 * 2^ceil(log2 T); k* = the lowest k with the largest A(nu_k). If 0 < k* < P and g(nu_{k*-1}) > 0 > g(nu_{k*+1}) the tune
 * is the root of g in that bracket (safeguarded Newton steps, every iterate inside the bracket, until the bracket or the step is
 * <= 2^-48; a fixed cap of steps), else nu_{k*}. The amplitude of the line is 2 |F(tune)| / sum w.
 *   nu[S][C], amp[S][C] (float64): C = the bits set in `columns` (bit 0: x, bit 1: y, bit 2: tau), in that order. The tune is in
 *   cycles per record step and lies in [0, 1/2].
 *   A = 0 on the whole grid: nu = NaN, amp = 0. A sample of the window that is not finite: NaN, NaN for that signal.
 *   lost[S] (int32, may be NULL): a row with 0 < lost <= last_turn (the turn number of the window's last record) is NaN, NaN.
 * k* comes from a float32 transform of P complex points in LDS, settled against its two neighbours in float64; everything else is
 * float64 sums in a fixed order (bitwise reproducible). One workgroup per row, no workspace, no host synchronisation.
 * CHX_ERR_INVALID_ARG before any launch: a NULL probe / nu / amp, R < 1, S < 1, r0 < 0, T outside CHX_TUNES_T_MIN .. CHX_TUNES_T_MAX,
 * r0 + T > R, columns outside 1 .. 7; CHX_ERR_DTYPE: dtype other than CHX_F32 / CHX_F64.
 * (An additive export: CHX_ABI_VERSION stays as it is.) */
#define CHX_TUNES_T_MIN 8
#define CHX_TUNES_T_MAX 4096
int chx_tunes(const void* probe, const int32_t* lost, int64_t R, int64_t S, int64_t r0, int64_t T, int64_t last_turn,
              int columns /* bit 0: x, bit 1: y, bit 2: tau */, int dtype, double* nu, double* amp /* (S, C) */, void* stream);
/* ---- short-range wakefield (Wakefield element): per batch row b, over the SURVIVING particles (w > 0, finite tau; c = |q| w):
 * tau_lo, tau_hi, node spacing D = (tau_hi - tau_lo) / (M - 1); node coordinate u = clamp((tau - tau_lo) / D, 0, M - 1) (0 when
 * D = 0), k = min(floor u, M - 2), f = u - k; node deposits Q_k += (1 - f) c, Q_k+1 += f c (and X, Y with c x, c y when the
 * transverse table is given); the tables wl[Ll] (V/C), wt[Lt] (V/(C m)) (fp64, entry n at s = n h[0]; Ll or Lt may be 0, not
 * both) sampled linearly at s = n D, 0 beyond the last entry, the n = 0 sample halved; V_k = -sum_{m<=k} Wl~_{k-m} Q_m,
 * U_k = sum_{m<=k} Wt~_{k-m} X_m (Y likewise); every particle (dead ones too; NaN tau -> NaN) gets
 * delta += scale[b] V(u), px += scale[b] Ux(u), py += scale[b] Uy(u) (linear interpolation, fp64, rounded once), scale[B]
 * fp64 = factor |Z| / p0c. A row without surviving particles is copied bit for bit. out[B][N][7], state[B][CHX_WAKE_STATE_DOUBLES(M)]
 * (the row header, node kicks and deposits the backward pass reads). x, q, w (dtype, [Bx][N][7], [Bq][N], [Bw][N]).
 * Deterministic: the deposits are 64-bit fixed-point sums (LDS then global integer atomics), scaled per row and channel from a
 * bound of the channel's total so that no sum overflows; every other reduction is in a fixed order. 2 <= M <= CHX_WAKE_MAX_BINS.
 * workspace: chx_wake_workspace_bytes(B, N, M) (also for the backward pass).
 * chx_wake_kick_bwd: given d_out[B][N][7] (dtype) and the forward's state -> dX[B][N][7], dC[B][N] (dtype; gradient with
 * respect to c, 0 for particles that do not deposit; may be NULL), d_scale[B], d_wl[Ll], d_wt[Lt] (fp64, summed over the rows;
 * each may be NULL). The node spacing is a constant (no gradient through tau_lo, tau_hi). Rows of broadcast inputs are NOT
 * reduced — the caller sums. */
#define CHX_WAKE_MAX_BINS 4096
#define CHX_WAKE_STATE_HEADER 8
#define CHX_WAKE_STATE_DOUBLES(M) (CHX_WAKE_STATE_HEADER + 6 * (int64_t)(M))
size_t chx_wake_workspace_bytes(int64_t B, int64_t N, int32_t M);
int chx_wake_kick(const void* x, const void* q, const void* w, const double* scale, const double* wl, int64_t Ll, const double* wt,
                  int64_t Lt, const double* h, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int32_t M, int dtype,
                  void* out, double* state, void* workspace, size_t workspace_bytes, void* stream);
int chx_wake_kick_bwd(const void* x, const void* q, const void* w, const double* scale, const double* wl, int64_t Ll,
                      const double* wt, int64_t Lt, const double* h, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N,
                      int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC, double* d_scale,
                      double* d_wl, double* d_wt, void* workspace, size_t workspace_bytes, void* stream);
/* ---- steady-state coherent synchrotron radiation (CSRKick element): per batch row b, the surviving particles' grid and node-based
 * linear deposit D_k (coulomb) exactly as chx_wake_kick's (same tau_lo, node spacing h, u, k, f, clamping, dead particles, NaN tau);
 * a_j = (j+1)^(2/3) - j^(2/3) in the cancellation-free form (2j+1) / ((j+1)^(4/3) + (j(j+1))^(2/3) + j^(4/3)), b_0 = -1, b_j = a_(j-1)
 * - a_j; S_k = sum_{j=0}^{M-1-k} b_j D_(k+j) (anti-causal: the sources are the particles behind, at larger tau); node energy change
 * dE_k [eV] = |Z| 3^(2/3) k_e L^(1/3) |theta|^(2/3) h^(-4/3) S_k (k_e = 8.9875517923e9 V m / C); every particle (dead ones too; NaN tau
 * -> NaN) gets delta += ((1 - f) dE_k + f dE_(k+1)) / p0c (fp64, rounded once; where the field is zero — theta = 0, L = 0, both nodes 0
 * — delta keeps its bits, NaN tau included). energy[Be], length[Bl] (L >= 0; a negative L gives NaN), angle[Ba] (theta) are device
 * arrays of the beam's dtype (each 1 or B rows); p0c = beta gamma m c^2 of the energy and the scale are formed on the device, in fp64.
 * A row without surviving particles or with h = 0 is copied bit for bit. out[B][N][7], state[B][CHX_CSR_STATE_DOUBLES(M)] (row header
 * as chx_wake_kick's with the row's scale |Z| L^(1/3) |theta|^(2/3) / p0c in its last slot, then the node kicks dE_k / (|Z| L^(1/3)
 * |theta|^(2/3))). x, q, w (dtype, [Bx][N][7], [Bq][N], [Bw][N]). Deterministic (64-bit fixed-point deposit, fixed-order sums). 2 <= M
 * <= CHX_WAKE_MAX_BINS. workspace: chx_csr_workspace_bytes(B, N, M) (also for the backward pass).
 * chx_csr_kick_bwd: given d_out[B][N][7] (dtype) and the forward's state -> dX[B][N][7] (delta's cotangent passes through), dC[B][N]
 * (dtype; gradient with respect to c = |q| w, 0 for particles that do not deposit; may be NULL) and d_scale[B] (fp64, gradient with
 * respect to the row's scale: the caller chains it to energy, L and theta). The node grid is a constant (no gradient through tau_lo,
 * h). Rows of broadcast inputs are NOT reduced — the caller sums. */
#define CHX_CSR_STATE_DOUBLES(M) (CHX_WAKE_STATE_HEADER + (int64_t)(M))
size_t chx_csr_workspace_bytes(int64_t B, int64_t N, int32_t M);
int chx_csr_kick(const void* x, const void* q, const void* w, const void* energy, const void* length, const void* angle,
                 double mass_eV, double abs_charge, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl,
                 int64_t Ba, int64_t N, int32_t M, int dtype, void* out, double* state, void* workspace, size_t workspace_bytes,
                 void* stream);
int chx_csr_kick_bwd(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int32_t M,
                     int dtype, const double* state, const void* d_out, void* dX, void* dC, double* d_scale, void* workspace,
                     size_t workspace_bytes, void* stream);
/* ---- entrance transient of coherent synchrotron radiation (TransientCSRKick element): chx_csr_kick's deposit, scale, gather and
 * degenerate cases with the kernel of a bunch that has travelled the arc length d into a bend behind a long straight (Saldin,
 * Schneidmiller, Yurkov, NIM A 398 (1997) 373): x = z_L / h = d^3 theta^2 / (24 L^2 h) (0, no kick, where L, theta or d is 0; NaN for a
 * negative L or d), a~_j = min(j+1, x)^(2/3) - min(j, x)^(2/3) (cancellation-free, 0 for j >= x), D~(y) the linear interpolation of
 * the deposits at the real index y (0 beyond node M),
 *   S_k = sum_j a~_j (D_(k+j+1) - D_(k+j)) - (2/3) x^(-1/3) [D~(k + x) - D~(k + 4x)],   dE_k = |Z| 3^(2/3) k_e L^(1/3) |theta|^(2/3) h^(-4/3) S_k
 * summed as a Toeplitz table b_j(x) in chx_csr_kick's order; for x >= M the table, and with it the result, is chx_csr_kick's bit for
 * bit. distance[Bd] (d) is a device array like length and angle. state[B][CHX_CSR_TRANSIENT_STATE_DOUBLES(M)]: the row header with
 * the scale in its last slot, the M node kicks, x, a free slot, the M deposits D_k. workspace:
 * chx_csr_transient_workspace_bytes(B, N, M) (also for the backward pass).
 * chx_csr_transient_kick_bwd: as chx_csr_kick_bwd, with d_x[B] (fp64) besides d_scale[B]: the gradient with respect to the row's x
 * (the node spacing h a constant), which the caller chains to L, theta and d; 0 where x = 0. */
#define CHX_CSR_TRANSIENT_STATE_DOUBLES(M) (CHX_WAKE_STATE_HEADER + 2 + 2 * (int64_t)(M))
size_t chx_csr_transient_workspace_bytes(int64_t B, int64_t N, int32_t M);
int chx_csr_transient_kick(const void* x, const void* q, const void* w, const void* energy, const void* length, const void* angle,
                           const void* distance, double mass_eV, double abs_charge, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw,
                           int64_t Be, int64_t Bl, int64_t Ba, int64_t Bd, int64_t N, int32_t M, int dtype, void* out, double* state,
                           void* workspace, size_t workspace_bytes, void* stream);
int chx_csr_transient_kick_bwd(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N,
                               int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC, double* d_scale,
                               double* d_x, void* workspace, size_t workspace_bytes, void* stream);
/* ---- coherent synchrotron radiation in the drift behind a bend (CSRDriftKick element): chx_csr_kick's deposit, gather and
 * degenerate cases with the wake of the radiation that was emitted inside a bend of length L_b and angle theta and catches up with the
 * bunch a distance x behind the bend's exit face (Stupakov and Emma, EPAC 2002, case D). With R = L_b / |theta|, phi = |theta|,
 * xh = x / R, kappa = 24 h / R, psi(u) the root of psi^3 (psi + 4 xh) / (psi + xh) = 24 u / R (12 Newton steps from the power of
 * two at or above (24 u / R)^(1/3) and one more), psi_j = min(psi(j h), phi), y = phi^3 (phi + 4 xh) / (kappa (phi + xh)) and
 * G(psi) = psi^2 / 2 + xh^2 psi / (psi + xh) - xh^2 log1p(psi / xh) (below psi / xh = 1/4 its series from the cubic term on),
 * the table a fixed sequence of IEEE operations (its own log1p; no library function),
 *   S_k = (1 / (2 h^2)) { sum_j [G(psi_(j+1)) - G(psi_j)] (D_(k+j+1) - D_(k+j)) - kappa / (3 (phi + 2 xh)) D~(k + y) },
 *   delta_k += (|Z| k_e L / p0c) S_k
 * with D~ the linear interpolation of the deposits at a real index and every deposit beyond node M equal to 0, summed as a Toeplitz
 * table in chx_csr_kick's order. length[Bl] (L, the piece of drift the kick stands for), bend_length[Bbl], bend_angle[Bba] and
 * distance[Bd] (x) are device arrays like chx_csr_kick's; no kick (the bits kept) where L, L_b or theta is 0, NaN for a negative L,
 * L_b or x. state[B][CHX_CSR_DRIFT_STATE_DOUBLES(M)]: the row header with the scale |Z| L / p0c in its last slot, the M node kicks
 * k_e S_k, then xh, phi, kappa, a free slot, the M deposits D_k. workspace: chx_csr_drift_workspace_bytes(B, N, M) (also for the
 * backward pass).
 * chx_csr_drift_kick_bwd: as chx_csr_kick_bwd, with d_xh[B], d_phi[B], d_kappa[B] (fp64) besides d_scale[B]: the gradients with
 * respect to the row's three shape numbers (the node spacing h and the lags floor(y), floor(y) + 1 constants), which the caller
 * chains to L_b, theta and x; 0 where there is no kick. */
#define CHX_CSR_DRIFT_STATE_DOUBLES(M) (CHX_WAKE_STATE_HEADER + 4 + 2 * (int64_t)(M))
size_t chx_csr_drift_workspace_bytes(int64_t B, int64_t N, int32_t M);
int chx_csr_drift_kick(const void* x, const void* q, const void* w, const void* energy, const void* length, const void* bend_length,
                       const void* bend_angle, const void* distance, double mass_eV, double abs_charge, int64_t B, int64_t Bx,
                       int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl, int64_t Bbl, int64_t Bba, int64_t Bd, int64_t N, int32_t M,
                       int dtype, void* out, double* state, void* workspace, size_t workspace_bytes, void* stream);
int chx_csr_drift_kick_bwd(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N,
                           int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC, double* d_scale,
                           double* d_xh, double* d_phi, double* d_kappa, void* workspace, size_t workspace_bytes, void* stream);
/* ---- longitudinal space charge (LSCKick element): per batch row b, the surviving particles' grid and node-based linear deposit D_k
 * (coulomb) exactly as chx_wake_kick's and chx_csr_kick's (same tau_lo, node spacing h, u, k, f, clamping, dead particles, NaN tau);
 * the on-axis field of a uniformly charged disc of radius a and Lorentz factor gamma, integrated exactly against the hat functions:
 * rho = a / (gamma h), P(v) = v / (|v| + sqrt(v^2 + rho^2)) + asinh(v / rho), c^_0 = 0, c^_(-j) = -c^_j, c^_j = -(P(j+1) - 2 P(j) +
 * P(j-1)) / 2; V_k = sum_{j=-k}^{M-1-k} c^_j D_(k+j) (two-sided: charge behind a witness, at larger tau, pushes it forward); every
 * particle (dead ones too; NaN tau -> NaN) gets delta += S ((1 - f) V_k + f V_(k+1)) with S = |Z| 2 k_e L / (gamma^2 h^2 p0c) (fp64,
 * rounded once; where the field is zero — L = 0, both nodes 0 — delta keeps its bits, NaN tau included). energy[Be], length[Bl] (L),
 * radius[Ba] (a) are device arrays of the beam's dtype (each 1 or B rows); gamma, p0c, S and rho are formed on the device, in fp64. A
 * row whose radius is not > 0 or not finite gets NaN in delta. A row without surviving particles or with h = 0 is copied bit for bit.
 * out[B][N][7], state[B][CHX_LSC_STATE_DOUBLES(M)] (row header as chx_wake_kick's with S in its last slot, the M node sums V_k, rho, a
 * free slot, the M deposits D_k). x, q, w (dtype, [Bx][N][7], [Bq][N], [Bw][N]). Deterministic (64-bit fixed-point deposit, fixed-order
 * sums). 2 <= M <= CHX_WAKE_MAX_BINS. workspace: chx_lsc_workspace_bytes(B, N, M) (also for the backward pass).
 * chx_lsc_kick_bwd: given d_out[B][N][7] (dtype) and the forward's state -> dX[B][N][7] (delta's cotangent passes through), dC[B][N]
 * (dtype; gradient with respect to c = |q| w, 0 for particles that do not deposit; may be NULL), d_scale[B] and d_rho[B] (fp64,
 * gradients with respect to the row's S and rho: the caller chains them to energy, L and a). The node grid is a constant (no gradient
 * through tau_lo, h). Rows of broadcast inputs are NOT reduced — the caller sums. */
#define CHX_LSC_STATE_DOUBLES(M) (CHX_WAKE_STATE_HEADER + 2 + 2 * (int64_t)(M))
size_t chx_lsc_workspace_bytes(int64_t B, int64_t N, int32_t M);
int chx_lsc_kick(const void* x, const void* q, const void* w, const void* energy, const void* length, const void* radius,
                 double mass_eV, double abs_charge, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl,
                 int64_t Ba, int64_t N, int32_t M, int dtype, void* out, double* state, void* workspace, size_t workspace_bytes,
                 void* stream);
int chx_lsc_kick_bwd(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int32_t M,
                     int dtype, const double* state, const void* d_out, void* dX, void* dC, double* d_scale, double* d_rho,
                     void* workspace, size_t workspace_bytes, void* stream);
/* ---- incoherent synchrotron radiation (SynchrotronRadiationKick element): the classical energy loss and the quantum excitation
 * (Gaussian approximation) of an arc of length L and bend angle theta, as one zero-length kick. Per batch row b, in fp64, with gamma0 =
 * energy / mass_eV, P0 = beta0 gamma0 (beta0 as `Beam.p0c`), r_c = abs_charge^2 r_e m_e / m, lambda_c = hbar c / mc^2:
 *   a = (2/3) r_c theta^2 / L,   b = 55 / (24 sqrt 3) r_c lambda_c |theta|^3 / L^2   (both 0 where L = 0 or theta = 0, NaN for L < 0)
 * and per particle n, in fp64 whatever the dtype, rounded once on the store:
 *   g = gamma0 + delta P0, pi = sqrt(g^2 - 1), g' = g - a P0^2 pi g - sqrt(b P0^3 g^7 / pi^3) xi,
 *   delta' = delta + (g' - g) / P0, px' = px pi' / pi, py' = py pi' / pi with pi' = sqrt(g'^2 - 1).
 * x, y, tau and the seventh column keep their bits; a row with a = b = 0 keeps every bit. A particle with a non-finite delta, px or
 * py, or with g' <= 1, gets NaN in delta', px', py'. quantum_excitation = 0: the xi term is absent and nothing is drawn.
 * xi = sqrt(-2 ln u1) cospi(2 u2), u1 = (((w0 2^32 + w1) >> 11) + 1/2) 2^-53, u2 likewise from (w2, w3), with (w0 .. w3) =
 * Philox4x32-10(counter = (n, b, call_lo, call_hi), key = (seed, rng_stream)), the standard multipliers and Weyl constants: xi of
 * particle n does not depend on N, the launch geometry or the dtype. call_index: ONE int64 in device memory, read by the kernel (a
 * captured graph follows it); the caller advances it. energy[Be], length[Bl], angle[Ba]: device arrays of the beam's dtype, each 1 or
 * B rows. x[Bx][N][7], out[B][N][7] (16-byte aligned). 1 <= B <= 65535, 1 <= N < 2^32, mass_eV > 0. Deterministic.
 * chx_sr_kick_bwd: the same arguments and d_out[B][N][7] (dtype) -> dX[B][N][7] and the per-row cotangents d_gamma[B], d_a[B], d_b[B]
 * (fp64) of (gamma0, a, b), P0 = sqrt(gamma0^2 - 1) folded into gamma0's: the caller chains them to energy, L and theta. xi is drawn
 * again from the same counter. The rows' sums are formed in a fixed order (per-workgroup partials in the workspace, then one
 * workgroup per row): bitwise reproducible, no float atomics. Rows of a broadcast x are NOT reduced — the caller sums. A particle
 * whose output is NaN has zero gradient. workspace: chx_sr_workspace_bytes(B, N) (0 for a shape out of range).
 * chx_sr_normals: the draw itself, words_out[B][N][4] (uint32, 16-byte aligned) and xi_out[B][N] (fp64), `call` by value. */
size_t chx_sr_workspace_bytes(int64_t B, int64_t N);
int chx_sr_kick(const void* x, const void* energy, const void* length, const void* angle, double mass_eV, double abs_charge,
                int quantum_excitation, uint32_t seed, uint32_t rng_stream, const int64_t* call_index, int64_t B, int64_t Bx,
                int64_t Be, int64_t Bl, int64_t Ba, int64_t N, int dtype, void* out, void* stream);
int chx_sr_kick_bwd(const void* x, const void* energy, const void* length, const void* angle, double mass_eV, double abs_charge,
                    int quantum_excitation, uint32_t seed, uint32_t rng_stream, const int64_t* call_index, int64_t B, int64_t Bx,
                    int64_t Be, int64_t Bl, int64_t Ba, int64_t N, int dtype, const void* d_out, void* dX, double* d_gamma,
                    double* d_a, double* d_b, void* workspace, size_t workspace_bytes, void* stream);
int chx_sr_normals(uint32_t seed, uint32_t rng_stream, uint64_t call, int64_t B, int64_t N, uint32_t* words_out, double* xi_out,
                   void* stream);
/* ---- intrabeam scattering (IBSKick element): the growth of the slice energy spread along the bunch, Bane's high-energy approximation
 * of the Bjorken-Mtingwa rate (EPAC 2002) without dispersion and with beta = 1, the bunch average N / sigma_s replaced by the local
 * line density. Per batch row b, the surviving particles' grid and node-based linear deposit D_k (coulomb) exactly as chx_lsc_kick's
 * (same tau_lo, node spacing h, u, k, f, clamping, dead particles); in fp64, with gamma = energy / mass_eV, r_c = abs_charge^2 r_e m_e / m:
 *   alpha = (sigma_x eps_y) / (sigma_y eps_x), g = sqrt(alpha) / AGM(1, alpha) (8 steps of (a, b) <- ((a + b) / 2, sqrt(a b)), result a),
 *   K = sqrt(pi) r_c^2 Lambda L g / (4 gamma^3 sqrt(eps_x eps_y sigma_x sigma_y) abs_charge e),   V_k = (K / h) D_k
 * and every particle (dead ones too) gets delta += sqrt(V(u)) xi with V(u) = (1 - f) V_k + f V_(k+1) (fp64, rounded once). Where V(u)
 * is 0 (both nodes empty, L = 0) delta keeps its bits; every other column always does. A NaN tau gives NaN unless both nodes are
 * empty. A row in which Lambda, sigma_x, sigma_y, eps_x or eps_y is not > 0 or not finite gets NaN in delta. A row without surviving
 * particles or with h = 0 is copied bit for bit. xi as chx_sr_kick's, with the counter (n, b + 2^31, call_lo, call_hi): bit 31 of the
 * second word keeps the draws apart from chx_sr_kick's at the same key and call index. call_index: ONE int64 in device memory, read
 * by the kernels (a captured graph follows it); the caller advances it. energy[Be], length[Bl], coulomb_log[Bc], sigma_x[Bsx],
 * sigma_y[Bsy], eps_x[Bex], eps_y[Bey] (geometric emittances, m): device arrays of the beam's dtype, each 1 or B rows.
 * out[B][N][7], state[B][CHX_IBS_STATE_DOUBLES(M)] (row header as chx_wake_kick's with K / h in its last slot, the M node variances
 * V_k, the M deposits D_k). 1 <= N < 2^31, 2 <= M <= CHX_WAKE_MAX_BINS. Deterministic (64-bit fixed-point deposit, fixed-order sums).
 * workspace: chx_ibs_workspace_bytes(B, N, M) (also for the backward pass).
 * chx_ibs_kick_bwd: given d_out[B][N][7] (dtype), the forward's state and the call index the forward used -> dX[B][N][7] (delta's
 * cotangent passes through; tau's through V(u) and through the deposit), dC[B][N] (dtype; gradient with respect to c = |q| w, 0 for
 * particles that do not deposit; may be NULL) and d_scale[B] (fp64, gradient with respect to the row's K / h: the caller chains it to
 * the seven settings). xi is drawn again. A particle whose V(u) is not > 0 has zero gradient through V. The node grid is a constant.
 * Bitwise reproducible, no float atomics. Rows of broadcast inputs are NOT reduced — the caller sums.
 * chx_ibs_normals: the draw itself, words_out[B][N][4] (uint32, 16-byte aligned) and xi_out[B][N] (fp64), `call` by value. */
#define CHX_IBS_STATE_DOUBLES(M) (CHX_WAKE_STATE_HEADER + 2 * (int64_t)(M))
size_t chx_ibs_workspace_bytes(int64_t B, int64_t N, int32_t M);
int chx_ibs_kick(const void* x, const void* q, const void* w, const void* energy, const void* length, const void* coulomb_log,
                 const void* sigma_x, const void* sigma_y, const void* eps_x, const void* eps_y, double mass_eV, double abs_charge,
                 uint32_t seed, uint32_t rng_stream, const int64_t* call_index, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw,
                 int64_t Be, int64_t Bl, int64_t Bc, int64_t Bsx, int64_t Bsy, int64_t Bex, int64_t Bey, int64_t N, int32_t M,
                 int dtype, void* out, double* state, void* workspace, size_t workspace_bytes, void* stream);
int chx_ibs_kick_bwd(const void* x, const void* q, const void* w, uint32_t seed, uint32_t rng_stream, const int64_t* call_index,
                     int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int32_t M, int dtype, const double* state,
                     const void* d_out, void* dX, void* dC, double* d_scale, void* workspace, size_t workspace_bytes, void* stream);
int chx_ibs_normals(uint32_t seed, uint32_t rng_stream, uint64_t call, int64_t B, int64_t N, uint32_t* words_out, double* xi_out,
                    void* stream);
/* ---- low-pass filter of the binned-beam kicks (the elements' `cutoff_wavelength`): a twin of each of the twelve calls above that takes
 * cutoff[Bcut] (fp64 device array of cutoff wavelengths lambda_c in metres, Bcut = 1 or B) in front of the workspace. Per batch row, with h
 * the row's node spacing, between the deposit and the node pass every deposited channel (Q; Q, X, Y of the wake) is smoothed:
 *   s = lambda_c / (2 pi h),  R = max(1, min(ceil(4 s), M - 1)),  g_d = exp(-d^2 / 2 s^2) / sum_{|e| <= R} g_e,
 *   D'_j = sum_{|d| <= R} g_d D_refl(j - d),  refl(i) = -1 - i for i < 0, 2 M - 1 - i for i >= M
 * (amplitude response exp(-(lambda_c / lambda)^2 / 2); symmetric, columns sum to 1: the charge is kept; no negative weight). The node
 * pass, the state and the gather see D'; the fixed-point scales are those of the deposit. The backward twins apply the same stage to
 * the deposits' cotangents before the last particle pass. A row without a grid (no survivor, h = 0) and a cutoff that is not > 0 or not
 * finite are left unfiltered; weights that are the identity (g_1 = 0) leave every bit. The cutoff is a constant: no gradient.
 * cutoff = NULL is the call without the suffix, bit for bit (which is how those are implemented), with that call's workspace. One more
 * launch each way (one workgroup per row, channel and 256 nodes; weights and window in LDS, fixed order, no atomics). The stage
 * writes a grid of its own, so a call with a cutoff needs chx_*_workspace_bytes_cut(B, N, M) (also for the backward pass): the
 * call's workspace and one more [B][channels][M] block of 8 bytes. */
size_t chx_wake_workspace_bytes_cut(int64_t B, int64_t N, int32_t M);
size_t chx_csr_workspace_bytes_cut(int64_t B, int64_t N, int32_t M);
size_t chx_csr_transient_workspace_bytes_cut(int64_t B, int64_t N, int32_t M);
size_t chx_csr_drift_workspace_bytes_cut(int64_t B, int64_t N, int32_t M);
size_t chx_lsc_workspace_bytes_cut(int64_t B, int64_t N, int32_t M);
size_t chx_ibs_workspace_bytes_cut(int64_t B, int64_t N, int32_t M);
int chx_lsc_kick_cut(const void* x, const void* q, const void* w, const void* energy, const void* length, const void* radius,
                     double mass_eV, double abs_charge, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl,
                     int64_t Ba, int64_t N, int32_t M, int dtype, void* out, double* state, const double* cutoff, int64_t Bcut,
                     void* workspace, size_t workspace_bytes, void* stream);
int chx_lsc_kick_bwd_cut(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N,
                         int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC, double* d_scale,
                         double* d_rho, const double* cutoff, int64_t Bcut, void* workspace, size_t workspace_bytes, void* stream);
int chx_csr_kick_cut(const void* x, const void* q, const void* w, const void* energy, const void* length, const void* angle,
                     double mass_eV, double abs_charge, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl,
                     int64_t Ba, int64_t N, int32_t M, int dtype, void* out, double* state, const double* cutoff, int64_t Bcut,
                     void* workspace, size_t workspace_bytes, void* stream);
int chx_csr_kick_bwd_cut(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N,
                         int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC, double* d_scale,
                         const double* cutoff, int64_t Bcut, void* workspace, size_t workspace_bytes, void* stream);
int chx_csr_transient_kick_cut(const void* x, const void* q, const void* w, const void* energy, const void* length,
                               const void* angle, const void* distance, double mass_eV, double abs_charge, int64_t B, int64_t Bx,
                               int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl, int64_t Ba, int64_t Bd, int64_t N, int32_t M,
                               int dtype, void* out, double* state, const double* cutoff, int64_t Bcut, void* workspace,
                               size_t workspace_bytes, void* stream);
int chx_csr_transient_kick_bwd_cut(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw,
                                   int64_t N, int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC,
                                   double* d_scale, double* d_x, const double* cutoff, int64_t Bcut, void* workspace,
                                   size_t workspace_bytes, void* stream);
int chx_csr_drift_kick_cut(const void* x, const void* q, const void* w, const void* energy, const void* length,
                           const void* bend_length, const void* bend_angle, const void* distance, double mass_eV, double abs_charge,
                           int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl, int64_t Bbl, int64_t Bba,
                           int64_t Bd, int64_t N, int32_t M, int dtype, void* out, double* state, const double* cutoff,
                           int64_t Bcut, void* workspace, size_t workspace_bytes, void* stream);
int chx_csr_drift_kick_bwd_cut(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw,
                               int64_t N, int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC,
                               double* d_scale, double* d_xh, double* d_phi, double* d_kappa, const double* cutoff, int64_t Bcut,
                               void* workspace, size_t workspace_bytes, void* stream);
int chx_wake_kick_cut(const void* x, const void* q, const void* w, const double* scale, const double* wl, int64_t Ll,
                      const double* wt, int64_t Lt, const double* h, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N,
                      int32_t M, int dtype, void* out, double* state, const double* cutoff, int64_t Bcut, void* workspace,
                      size_t workspace_bytes, void* stream);
int chx_wake_kick_bwd_cut(const void* x, const void* q, const void* w, const double* scale, const double* wl, int64_t Ll,
                          const double* wt, int64_t Lt, const double* h, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N,
                          int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC, double* d_scale,
                          double* d_wl, double* d_wt, const double* cutoff, int64_t Bcut, void* workspace, size_t workspace_bytes,
                          void* stream);
int chx_ibs_kick_cut(const void* x, const void* q, const void* w, const void* energy, const void* length, const void* coulomb_log,
                     const void* sigma_x, const void* sigma_y, const void* eps_x, const void* eps_y, double mass_eV,
                     double abs_charge, uint32_t seed, uint32_t rng_stream, const int64_t* call_index, int64_t B, int64_t Bx,
                     int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl, int64_t Bc, int64_t Bsx, int64_t Bsy, int64_t Bex, int64_t Bey,
                     int64_t N, int32_t M, int dtype, void* out, double* state, const double* cutoff, int64_t Bcut, void* workspace,
                     size_t workspace_bytes, void* stream);
int chx_ibs_kick_bwd_cut(const void* x, const void* q, const void* w, uint32_t seed, uint32_t rng_stream, const int64_t* call_index,
                         int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int32_t M, int dtype, const double* state,
                         const void* d_out, void* dX, void* dC, double* d_scale, const double* cutoff, int64_t Bcut,
                         void* workspace, size_t workspace_bytes, void* stream);
/* ---- laser energy modulation in an undulator (LaserModulator element; Huang et al., PRSTAB 7, 074401 (2004), eq. 8), as one
 * zero-length kick. Per batch row b, in fp64, with gamma0 = energy / mass_eV, P0 = beta0 gamma0 (as chx_sr_kick forms them), the
 * amplitude A (eV), the wavelength lambda, the phase phi, the rms size sigma_r of the laser intensity, the laser axis (x0, y0), the rms
 * length sigma_t of the intensity envelope and its centre tau0:
 *   a = A / (P0 mass_eV), nu = 1 / lambda, phi_t = phi / fl(2 pi), g = 1 / (4 sigma_r^2), h = 1 / (4 sigma_t^2)
 * (h = 0 for pulse_sigma = NULL: no envelope), and per particle n, in fp64 whatever the dtype, rounded once on the store, with
 * u = x - x0, v = y - y0, w = tau - tau0:
 *   t = fl(fl(tau nu) + phi_t) (turns; product and sum rounded separately), f = t - rint(t), Ex = exp(-g (u^2 + v^2) - h w^2),
 *   delta' = delta + a Ex sin(2 pi f), the sine as sincospi(2 f).
 * Every other column keeps its bits; a row with a = 0 keeps every bit. A particle whose x, y, tau or delta is not finite gets a
 * non-finite delta' (NaN, or the non-finite delta itself) and nothing else of it changes. energy[Be], amplitude[Ba], wavelength[Bw],
 * phase[Bp], laser_sigma[Bs], offset_x[Bx0], offset_y[By0], pulse_sigma[Bps] (or NULL), pulse_center[Bpc]: device arrays of the
 * beam's dtype, each 1 or B rows. x[Bx][N][7], out[B][N][7] (16-byte aligned). 1 <= B <= 65535, 1 <= N < 2^32, mass_eV > 0.
 * chx_laser_kick_bwd: the same arguments and d_out[B][N][7] (dtype) -> dX[B][N][7] and d_rows[B][8] (fp64), the per-row cotangents of
 * (a, nu, phi_t, g, x0, y0, h, tau0): the caller chains them to the energy and the eight settings. With G the cotangent of delta',
 * S = a Ex and (s, c) = sincospi(2 f): dX = d_out, x's adds -2 g u G S s, y's -2 g v G S s, tau's G S (2 pi nu c - 2 h w s); G_a =
 * sum G Ex s, G_nu = sum 2 pi tau G S c, G_phit = sum 2 pi G S c, G_g = -sum G S s (u^2 + v^2), G_x0 = sum 2 g u G S s, G_y0 = sum
 * 2 g v G S s, G_h = -sum G S s w^2, G_tau0 = sum 2 h w G S s. The rows' sums are formed in a fixed order (per-workgroup partials in
 * the workspace, then one workgroup per row): bitwise reproducible, no float atomics. Rows of a broadcast x are NOT reduced — the
 * caller sums. A particle whose delta' is not finite has zero gradient in the delta column and adds nothing. workspace:
 * chx_laser_workspace_bytes(B, N) (0 for a shape out of range). */
size_t chx_laser_workspace_bytes(int64_t B, int64_t N);
int chx_laser_kick(const void* x, const void* energy, const void* amplitude, const void* wavelength, const void* phase,
                   const void* laser_sigma, const void* offset_x, const void* offset_y, const void* pulse_sigma,
                   const void* pulse_center, double mass_eV, int64_t B, int64_t Bx, int64_t Be, int64_t Ba, int64_t Bw, int64_t Bp,
                   int64_t Bs, int64_t Bx0, int64_t By0, int64_t Bps, int64_t Bpc, int64_t N, int dtype, void* out, void* stream);
int chx_laser_kick_bwd(const void* x, const void* energy, const void* amplitude, const void* wavelength, const void* phase,
                       const void* laser_sigma, const void* offset_x, const void* offset_y, const void* pulse_sigma,
                       const void* pulse_center, double mass_eV, int64_t B, int64_t Bx, int64_t Be, int64_t Ba, int64_t Bw,
                       int64_t Bp, int64_t Bs, int64_t Bx0, int64_t By0, int64_t Bps, int64_t Bpc, int64_t N, int dtype,
                       const void* d_out, void* dX, double* d_rows, void* workspace, size_t workspace_bytes, void* stream);
/* ---- quiet-start deviates: out[N][D] (dtype) holds the Halton sequence in the D bases bases[D] (a HOST array read during the call;
 * distinct primes <= 19), as uniforms in (0, 1) (normal = 0) or as standard-normal deviates. Row n has the index i = offset + 1 + n;
 * index 0 is never used. 1 <= D <= CHX_QUIET_MAX_DIMS, N >= 1, offset >= 0, offset + N < 2^40 (CHX_ERR_INVALID_ARG otherwise, before
 * any device work). Radical inverse: in unsigned 64-bit integers the digits of i are peeled off in base b, r = r b + digit and
 * p = p b per digit; u = (double)r / (double)p, one IEEE division (r, p < 2^53: the same bits on any machine). Normal deviates, in
 * fp64: s = min(u, 1 - u), z = -+ sqrt(2) erfcinv(2 s), negative for u < 1/2, exactly 0 at u = 1/2. A float32 output is the fp64 value
 * rounded once on the store. One launch; bitwise reproducible; rows [a, b) of one call equal a call with offset + a. */
#define CHX_QUIET_MAX_DIMS 8
int chx_quiet_sequence(const int* bases, int64_t D, int64_t N, int64_t offset, int normal, int dtype, void* out, void* stream);
/* ---- seeded density modulation (ParticleBeam.with_density_modulation): the longitudinal density times 1 + sum_m A_m cos(2 pi tau /
 * lambda_m + phi_m), 1 <= K <= CHX_DENSITY_MAX_MODES modes: every particle's tau moves to the root tau' of
 *   tau' + sum_m c_m sin(2 pi (tau' nu_m + phi_t,m)) = tau,   nu_m = 1 / lambda_m, phi_t,m = phi_m / fl(2 pi), c_m = A_m / (fl(2 pi) nu_m),
 * in fp64 whatever the dtype, rounded once on the store. amplitudes[Ba][K], wavelengths[Bw][K], phases[Bp][K]: fp64 device arrays of 1
 * or B rows. The phase of mode m at t in turns: w = fl(fl(t nu_m) + phi_t,m), f = w - rint(w), sincospi(2 f). Solver: at most 32
 * steps from t = tau; the bracket [lo, hi], from tau -+ sum |c_m|, takes t on the side of the sign of g = t + sum c_m sin theta_m - tau
 * (theta_m the phase of mode m at t), and the step is Newton's t - g / D, D = 1 + sum A_m cos theta_m, where that stays inside the bracket and the bracket's middle otherwise; a particle
 * is done after a Newton step no longer than 2^-30 / max |nu_m| (the next error is its square: below 10^-16 wavelengths).
 * Every column but tau keeps its bits; a row whose A_m are all 0 keeps every bit; a non-finite tau stays as it is; in a row with
 * sum |A_m| >= 1 (or NaN), where the root is not unique, every finite tau becomes NaN. x[Bx][N][7], out[B][N][7] (16-byte aligned).
 * 1 <= B <= 65535, 1 <= N < 2^32.
 * chx_density_modulate_bwd: the same arguments and d_out[B][N][7] (dtype) -> dX[B][N][7] and d_rows[B][3][CHX_DENSITY_MAX_MODES] (fp64),
 * the per-row cotangents of (A_m, nu_m, phi_t,m), 0 for m >= K: the caller chains them to the settings. With G the cotangent of tau'
 * and theta_m the phase of mode m at tau' (solved again from x): dX = d_out, tau's column G / D; G_A,m = -sum G sin theta_m / (2 pi
 * nu_m D), G_nu,m = sum G (A_m sin theta_m / (2 pi nu_m^2) - A_m tau' cos theta_m / nu_m) / D, G_phit,m = -sum G A_m cos theta_m /
 * (nu_m D). The rows' sums are formed in a fixed order (per-workgroup partials in the workspace, then one workgroup per row): bitwise
 * reproducible, no float atomics. Rows of a broadcast x are NOT reduced — the caller sums. A particle whose tau' is not finite has
 * zero gradient in the tau column and adds nothing. workspace: chx_density_workspace_bytes(B, N) (0 for a shape out of range). */
#define CHX_DENSITY_MAX_MODES 8
size_t chx_density_workspace_bytes(int64_t B, int64_t N);
int chx_density_modulate(const void* x, const double* amplitudes, const double* wavelengths, const double* phases, int64_t K, int64_t B,
                         int64_t Bx, int64_t Ba, int64_t Bw, int64_t Bp, int64_t N, int dtype, void* out, void* stream);
int chx_density_modulate_bwd(const void* x, const double* amplitudes, const double* wavelengths, const double* phases, int64_t K,
                             int64_t B, int64_t Bx, int64_t Ba, int64_t Bw, int64_t Bp, int64_t N, int dtype, const void* d_out,
                             void* dX, double* d_rows, void* workspace, size_t workspace_bytes, void* stream);
/* Backward of chx_moments(y), y_n = R x_n, with respect to the MAP R[BR][7][7] (dtype) when the particles x carry no
 * gradient: mu' = A mu + b, cov' = A C A^T (element.py:180-191 + utils/statistics.py:4-62), so
 * dR[B][7][7] (double) = [2 G A C + g_mu mu^T | g_mu; 0] from d_out[B][29] and the INCOMING beam's chx_moments
 * mom_x[Bm][29] alone — no pass over the particles (tests/test_differentiable.py:10-32: d sigma_x(screen) / d k1). */
int chx_moments_mapped_bwd(const double* d_out, const void* R, const double* mom_x, int64_t B, int64_t BR, int64_t Bm,
                           int dtype, double* dR, void* stream);
/* One entry of the moment vector as a beam property reads it (particle_beam.py:1672-1943: mu_*, sigma_* = sqrt of the
 * variance, cov_*): out[b] (dtype) = mom[b][index] or its square root — and its backward for a linearly tracked beam in one
 * launch: grad[B] (dtype) of that entry -> dR[B][7][7] (double, or dtype when dR_is_double = 0) through
 * chx_moments_mapped_bwd's algebra; mom_y[B][29] = chx_moments of the tracked beam (for the square root). */
int chx_moment_entry(const double* mom, int64_t B, int index, int take_sqrt, int dtype, void* out, void* stream);
int chx_moment_entry_mapped_bwd(const void* grad, const double* mom_y, int index, int take_sqrt, const void* R,
                                const double* mom_x, int64_t B, int64_t BR, int64_t Bm, int dtype, void* dR, int dR_is_double,
                                void* stream);
/* Fused observables: out[b] = chx_moments of the tracked beam R[b] x without ever
 * writing it (element.py:180-191 followed by particle_beam.py:1672-1943), e.g. sigma_x(k1) over a scan of B
 * settings on one shared beam. One pass; second moments are accumulated about c_b = R[b] centre, where
 * centre[Bx][6] (double, device; e.g. the incoming means from chx_moment_sums) must lie within a few sigma of the
 * incoming mean (NULL = origin). y = R x is evaluated exactly like chx_apply_affine7 (same fma chain).
 * With a shared beam (Bx == Bw == 1, BR == B >= 64) each lane owns one batch row: no reduction across lanes. */
size_t chx_track_moments_workspace_bytes(int64_t B, int64_t N);
int chx_track_moments(const void* x_in, const void* w, const void* R, const double* centre, int64_t B, int64_t Bx,
                      int64_t BR, int64_t Bw, int64_t N, int dtype, double* out, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- cloud-in-cell deposition (a12; utils/cloud_in_cell.py:8-451) and Screen images
 * (a11; screen.py:241-344). Positions are read straight out of the particle array:
 * pos_d = (x[b][n][col[d]] * scale[b][d]) - shift[b][d], each step rounded in `dtype`
 * exactly like the reference's tensor ops (screen.py:200-212 misalignment subtraction,
 * particle_beam.py:1333 z = tau * -beta). Weight = charge * survival (|charge| if abs_charge).
 * Index arithmetic follows cloud_in_cell.py:150-211 in `dtype`, bit-exact. */
typedef struct chx_cic_args {
    int32_t ndim;            /* 1..3 */
    int32_t cols[3];         /* column of the 7-vector used for each axis */
    int32_t bins[3];         /* grid shape */
    int64_t grid_strides[3]; /* element strides of the output grid per axis (row-major default if 0) */
    int64_t grid_batch_stride;
    int64_t B, Bx, Bq, Bs, Be, Bsc, Bsh, N;
    int32_t dtype;
    int32_t abs_charge;
    const void* x;        /* [Bx][N][7] */
    const void* charge;   /* [Bq][N] or NULL (=1) */
    const void* survival; /* [Bs][N] or NULL (=1) */
    const void* extent;   /* [Be][ndim][2] (left,right) */
    const void* scale;    /* [Bsc][ndim] or NULL */
    const void* shift;    /* [Bsh][ndim] or NULL */
    void* grid;           /* [B] grids, dtype, accumulated into (caller zeroes) */
} chx_cic_args;
int chx_cic_deposit(const chx_cic_args* args, void* stream);
/* Fused "track, then deposit" (SURVEY section 8 row f2): the position of particle n in batch row b is taken from R[b] x
 * (R[BR][7][7], BR in {1, B}; coordinate cols[d] of the product, the fma chain of chx_apply_affine7 — bit-identical to
 * chx_apply_affine7 followed by chx_cic_deposit) without the (B, N, 7) tracked array ever being written: Screen images
 * for a scan of B lattice settings over one shared beam (element.py:180-191 + screen.py:327-339). */
int chx_cic_deposit_mapped(const chx_cic_args* args, const void* R, int64_t BR, void* stream);
/* Same result as chx_cic_deposit (identical addends, different summation order) for ndim 2 or 3 and large
 * N: particles are counting-sorted by grid tile, accumulated in LDS (ds_add) and flushed once per tile,
 * instead of 2^ndim global float atomics per particle (which saturate at ~21 G atomics/s on MI355X). */
size_t chx_cic_sorted_workspace_bytes(const chx_cic_args* args);
int chx_cic_deposit_sorted(const chx_cic_args* args, void* workspace, size_t workspace_bytes, void* stream);
/* The same deposit with grid = deposit instead of grid += deposit: every cell of every grid row is stored by the tile
 * that owns it (zeros included), so the caller does not zero the grid first and the flush carries no dependent load.
 * Used by chx_sc_kick (space_charge_kick.py:556-563 deposits into a fresh zero tensor). */
int chx_cic_deposit_sorted_overwrite(const chx_cic_args* args, void* workspace, size_t workspace_bytes, void* stream);
/* Test/diagnostic twin: writes the integer cell index i_d=floor(p_d) (int32 [B][N][ndim])
 * and fractional part f_d (dtype [B][N][ndim]) instead of depositing. */
int chx_cic_indices(const chx_cic_args* args, int32_t* idx_out, void* frac_out, void* stream);
/* Backward of the deposit wrt charges and positions (cloud_in_cell.py is differentiable):
 * dq[b][n] = sum_corners dgrid*weight ; dpos[b][n][d] via d(weight)/d(f_d) / bin_width. */
int chx_cic_deposit_bwd(const chx_cic_args* args, const void* dgrid, void* dweight /*[B][N]*/,
                        void* dpos /*[B][N][ndim]*/, void* stream);

/* Screen "histogram" method (screen.py:292-311 -> torch.histogramdd): bin j iff
 * e_j <= v < e_{j+1}, last bin right-inclusive, outside dropped; edges from torch.linspace. */
typedef struct chx_hist2d_args {
    int64_t B, Bx, Bq, Bs, Bsh, N;
    int32_t nx, ny; /* number of bins; edges have nx+1 / ny+1 entries */
    int32_t dtype;
    const void* x;        /* [Bx][N][7]; x = col 0, y = col 2 */
    const void* charge;   /* |charge| * survival is the weight */
    const void* survival;
    const void* shift;    /* [Bsh][2] screen misalignment or NULL */
    const void* edges_x;  /* [nx+1] dtype */
    const void* edges_y;  /* [ny+1] dtype */
    void* image;          /* [B][ny][nx] dtype (already transposed like screen.py:311), caller zeroes */
} chx_hist2d_args;
int chx_hist2d(const chx_hist2d_args* args, void* stream);
int chx_hist2d_indices(const chx_hist2d_args* args, int32_t* ij_out /*[B][N][2], -1 = dropped*/,
                       void* stream);

/* Derivatives of the space-charge kick (the reference differentiates space_charge_kick.py with torch autograd;
 * tests/test_space_charge_kick.py:202-327). Together with chx_cic_deposit_bwd, chx_moments' backward and the
 * self-adjoint chx_sc_convolve they make SpaceChargeKick.track differentiable on power-of-two grids.
 *  - chx_sc_igf_table_grad: tables[3][B][(gx+1)(gy+1)(gz+1)] (double) = d(corner table of chx_sc_igf_table) /
 *    d(cell_x, cell_y, cell_z * gamma); feeding each through chx_sc_green_spectrum + chx_sc_convolve gives
 *    d phi / d(that cell size), so dL/dcell = sum(dphi * that).
 *  - chx_sc_gradient_bwd: dphi[B][gx][gy][gz] = adjoint of chx_sc_gradient (compact phi) applied to dF[B][g^3][4].
 *  - chx_sc_gather_kick_bwd: dx[B][N][7] (may be NULL); dF[B][g^3][4] (may be NULL; ACCUMULATED with atomics — the
 *    caller zero-fills); partials (may be NULL) = chx_sc_gather_kick_bwd_partials_count() doubles
 *    [B][ceil(N/256)][8] = per-workgroup sums of dY . d x_out / d (half[3], cell[3], dt, energy). */
int chx_sc_igf_table_grad(const void* cell, const void* gamma, int64_t B, const int32_t* bins, int dtype, double* tables,
                          void* stream);
int chx_sc_gradient_bwd(const void* dF, const void* cell, const void* gamma, int64_t B, const int32_t* bins, int dtype,
                        void* dphi, void* stream);
int64_t chx_sc_gather_kick_bwd_partials_count(int64_t B, int64_t N);
int chx_sc_gather_kick_bwd(const void* x_in, const void* F, const void* half, const void* cell, const void* energy,
                           const void* dt, const void* dY, double mass_eV, int64_t B, int64_t Bx, int64_t Be, int64_t N,
                           const int32_t* bins, int dtype, void* dx, void* dF, double* partials, void* stream);

/* Screen "kde" method (screen.py:312-326, utils/kde.py:4-77): Gaussian kernel values of particles n0 .. n0 + nchunk - 1
 * against the bin centres,  out[B][nchunk][nbins] = max(w exp(-((v - c_i) / sigma)^2 / 2) / sqrt(2 pi sigma^2), tiny),
 * v = x[..][col] - shift (col 0: x, col 2: y), w = |charge| * survival (either may be NULL = 1). The joint density is
 * the GEMM of two such arrays over the particle axis, left to the BLAS library by the host layer. */
int chx_kde_values(const void* x, const void* charge, const void* survival, const void* shift, const void* centres,
                   const void* sigma, int col, int64_t B, int64_t Bx, int64_t Bq, int64_t Bs, int64_t Bsh, int64_t N,
                   int64_t n0, int64_t nchunk, int32_t nbins, int dtype, void* out, void* stream);

/* ---- space charge (a13; space_charge_kick.py:103-586, particle_beam.py:1262-1346) */
/* Integrated Green function on the doubled grid (space_charge_kick.py:163-291).
 * cell[B][3] (dtype) = cell sizes (hx,hy,htau); gamma[B] (dtype). fp64 inside; the workspace
 * holds the (gx+1)(gy+1)(gz+1) corner table of the primitive per batch row. */
size_t chx_sc_igf_workspace_bytes(int64_t B, const int32_t* bins);
/* ldz = distance between rows of the last axis of G_out: 2gz (0 = default), or 2gz + 2 for the padded layout of
 * an in-place real-to-complex transform (chx_sc_fft_exec). */
int chx_sc_igf(const void* cell, const void* gamma, int64_t B, const int32_t* bins, int dtype,
               void* G_out /*[B][2gx][2gy][ldz]*/, int64_t ldz, void* workspace, size_t workspace_bytes,
               void* stream);
/* The same doubled array from a corner table that already exists (chx_sc_igf_table, or one of the three derivative tables of
 * chx_sc_igf_table_grad — the backward pass of the Poisson stage on grids outside chx_sc_pruned_supported). */
int chx_sc_igf_from_table(const double* table, int64_t B, const int32_t* bins, int dtype, void* G_out, int64_t ldz, void* stream);
/* 3-D FFTs of the Hockney convolution (space_charge_kick.py:306-314) through hipFFT, in place on the padded real
 * layout [B][2gx][2gy][2gz + 2] (= complex [B][2gx][2gy][gz + 1]), unnormalised. direction 0 / 1: forward with
 * plan 0 / 1 (two plans, so rho and the Green function can be transformed concurrently on two streams),
 * 2: inverse. Plan creation is a host-side call that may allocate hipFFT work areas; exec only enqueues. */
int chx_sc_fft_plan_create(int64_t B, const int32_t* bins, int dtype, void** plan_out);
int chx_sc_fft_plan_destroy(void* plan);
int chx_sc_fft_exec(void* plan, int direction, void* data, void* stream);
/* Pruned, symmetry-aware Poisson solve (csrc/chx_fft.hip) for power-of-two grids (chx_sc_pruned_supported):
 *  - chx_sc_igf_table: the (gx+1)(gy+1)(gz+1) corner table of the Green-function primitive (double);
 *  - chx_sc_green_spectrum: real, even spectrum of the integrated Green function on the doubled grid, stored on
 *    (gx+1)(gy+1)(gz+1) points (the spectrum at index k and 2g-k is the same number);
 *  - chx_sc_convolve: phi[B][gx][gy][gz] = crop(ifft(fft(pad(rho)) * Ghat * scale[b])) from the COMPACT rho[B][gx][gy][gz]:
 *    the zero padding is implicit (the zero halves of the lines are never read) and only the first octant of the
 *    result is ever written; transforms unnormalised (fold 1/(8 gx gy gz) into scale). */
int chx_sc_pruned_supported(const int32_t* bins, int dtype);
int chx_sc_igf_table(const void* cell, const void* gamma, int64_t B, const int32_t* bins, int dtype, double* table,
                     void* stream);
size_t chx_sc_green_workspace_bytes(int64_t B, const int32_t* bins, int dtype);
/* chx_sc_igf_table + chx_sc_green_spectrum in one call from cell[B][3] / gamma[B] (dtype). fp32 grids evaluate the
 * 6-transcendental primitive (space_charge_kick.py:103-123) only for cells closer than 8 x the largest cell edge and use
 * the 4th-order multipole expansion of the cell integral of 1/r beyond (relative error <= 1e-8, below fp32 rounding);
 * fp64 grids are exact everywhere. */
size_t chx_sc_green_fast_workspace_bytes(int64_t B, const int32_t* bins, int dtype);
int chx_sc_green_spectrum_fast(const void* cell, const void* gamma, int64_t B, const int32_t* bins, int dtype, void* Ghat,
                               void* workspace, size_t workspace_bytes, void* stream);
int chx_sc_green_spectrum(const double* table, int64_t B, const int32_t* bins, int dtype, void* Ghat, void* workspace,
                          size_t workspace_bytes, void* stream);
size_t chx_sc_convolve_workspace_bytes(int64_t B, const int32_t* bins, int dtype);
int chx_sc_convolve(const void* rho, const void* Ghat, const double* scale, int64_t B, const int32_t* bins, int dtype,
                    void* phi, void* workspace, size_t workspace_bytes, void* stream);
/* The same convolution with the potential stored inside a halo of 2 nodes: phi_halo[B][gx+4][gy+4][gz+4] (dtype,
 * chx_sc_phi_halo_elements() elements), node (i, j, k) at [i+2][j+2][k+2]. The halo itself is NOT written; its content is
 * undefined and chx_sc_gather_kick_phi reads it only where the value is discarded. Workspace as chx_sc_convolve. */
size_t chx_sc_phi_halo_elements(int64_t B, const int32_t* bins);
int chx_sc_convolve_halo(const void* rho, const void* Ghat, const double* scale, int64_t B, const int32_t* bins, int dtype,
                         void* phi_halo, void* workspace, size_t workspace_bytes, void* stream);
/* The same convolution (space_charge_kick.py:262-322: FFT of the padded charge, product with the Green spectrum, inverse FFT,
 * crop), for a Green spectrum that another stream is still computing: `ghat_ready_event` (a hipEvent_t recorded on that
 * stream behind the spectrum, or NULL) is waited for on `stream` in front of the pass that first reads Ghat — the forward
 * x and y passes of rho do not wait. */
int chx_sc_convolve_halo_after(const void* rho, const void* Ghat, const double* scale, int64_t B, const int32_t* bins, int dtype,
                               void* phi_halo, void* workspace, size_t workspace_bytes, void* stream, void* ghat_ready_event);
/* Grid geometry of a kick from the beam moments (space_charge_kick.py:531-550,110-130), one launch instead of ~25
 * tensor ops: moments[Bm][29] (chx_moments layout), grid_extent[Bext][3] (in sigmas), energy[Be], length[Bl] ->
 * half[B][3] = extent*sigma, cell[B][3] = 2 half / bins, gamma[B], dt[B] = L/(c beta), scale[B][3] = (1, 1, -beta),
 * extent[B][3][2] = (-half, half) (all `dtype`, rounded step by step like the reference's tensor expressions) and
 * pot_scale[B] (double) = pot_factor / prod(cell). */
int chx_sc_geometry(const double* moments, const void* grid_extent, const void* energy, const void* length,
                    double mass_eV, double pot_factor, int64_t B, int64_t Bm, int64_t Bext, int64_t Be, int64_t Bl,
                    const int32_t* bins, int dtype, void* half, void* cell, void* gamma, void* dt, void* scale,
                    void* extent, double* pot_scale, void* stream);
/* rho_hat *= G_hat * scale[b]  (complex multiply; space_charge_kick.py:313-316);
 * n_complex = complex elements per batch row; scale (double[B]) folds 1/(4 pi eps0), 1/cell volume and the FFT
 * normalisation. */
int chx_sc_spectral_mul(void* rho_hat, const void* G_hat, const double* scale, int64_t B,
                        int64_t n_complex, int dtype, void* stream);
/* E+vxB force field from the potential (space_charge_kick.py:324-365): central differences, x -1/gamma^2;
 * phi is the doubled array phi[B][2gx][2gy][ldz] (cropped on the fly, phi_doubled = 1; ldz = 0 means 2gz) or the
 * compact phi[B][gx][gy][gz] (phi_doubled = 0); F_out[B][gx][gy][gz][4]. */
int chx_sc_gradient(const void* phi, const void* cell, const void* gamma, int64_t B,
                    const int32_t* bins, int phi_doubled, int64_t ldz, int dtype, void* F_out, void* stream);
/* Fused: to_xyz_pxpypz -> trilinear node-based gather -> p += F*dt -> from_xyz_pxpypz
 * (space_charge_kick.py:387-475,548-584; particle_beam.py:1262-1346).
 * half[B][3] grid half-widths, cell[B][3], energy[Be], dt[B] (all dtype). */
int chx_sc_gather_kick(const void* x_in, const void* F, const void* half, const void* cell,
                       const void* energy, const void* dt, double mass_eV, int64_t B, int64_t Bx,
                       int64_t Be, int64_t N, const int32_t* bins, int dtype, void* x_out,
                       void* stream);
/* chx_sc_gather_kick followed by chx_apply_affine7 with post_map[BR][7][7] (BR in {1, B}) in ONE pass: the linear run that
 * follows a SpaceChargeKick inside a Segment (segment.py:545-574) is applied while the kicked particle is still in registers
 * (the kicked coordinates are rounded to dtype first, then the apply kernel's fma chain: bit-identical to the two passes).
 * chx_sc_kick takes the same optional map as its last arguments (NULL = kick only). */
int chx_sc_gather_kick_mapped(const void* x_in, const void* F, const void* half, const void* cell, const void* energy,
                              const void* dt, double mass_eV, int64_t B, int64_t Bx, int64_t Be, int64_t N, const int32_t* bins,
                              int dtype, const void* post_map, int64_t BR, void* x_out, void* stream);
/* chx_sc_gradient + chx_sc_gather_kick(_mapped) in ONE pass, without the force grid: every particle takes the central
 * differences of chx_sc_gradient (space_charge_kick.py:324-385; zero normal component on the boundary nodes) on the 32
 * potential values around its cell — phi_halo from chx_sc_convolve_halo, gamma[B] and cell[B][3] as for chx_sc_gradient —
 * in the same arithmetic and order, then interpolates and kicks: bit-identical to the two-kernel form, which writes and
 * re-reads a [g^3][4] force grid four times the size of the potential. post_map may be NULL (kick only). */
int chx_sc_gather_kick_phi(const void* x_in, const void* phi_halo, const void* half, const void* cell, const void* gamma,
                           const void* energy, const void* dt, double mass_eV, int64_t B, int64_t Bx, int64_t Be, int64_t N,
                           const int32_t* bins, int dtype, const void* post_map, int64_t BR, void* x_out, void* stream);
/* chx_moments + chx_sc_geometry for the kick: only the three variances the grid needs (sigma_x, sigma_y, sigma_tau;
 * space_charge_kick.py:531-538) are accumulated (8 fp64 sums per lane instead of 29, same shifted one-pass formulas and
 * rounding), and the partial sums are finalised inside the geometry kernel: two launches. Outputs as chx_sc_geometry. */
size_t chx_sc_beam_geometry_workspace_bytes(int64_t B, int64_t N);
int chx_sc_beam_geometry(const void* x, const void* w, const void* grid_extent, const void* energy, const void* length,
                         double mass_eV, double pot_factor, int64_t B, int64_t Bx, int64_t Bw, int64_t Bext, int64_t Be,
                         int64_t Bl, int64_t N, const int32_t* bins, int dtype, void* half, void* cell, void* gamma, void* dt,
                         void* scale, void* extent, double* pot_scale, void* workspace, size_t workspace_bytes, void* stream);
/* A whole SpaceChargeKick.track in ONE call (space_charge_kick.py:477-586) for grids chx_sc_pruned_supported() accepts:
 * chx_sc_beam_geometry -> [side stream: chx_sc_green_spectrum_fast] -> chx_cic_deposit_sorted_overwrite (N >= 65536; zero +
 * chx_cic_deposit below) -> chx_sc_convolve_halo -> chx_sc_gather_kick_phi, all intermediates in `workspace`
 * (chx_sc_kick_workspace_bytes). x_in[Bx][N][7], charge[Bq][N], survival[Bs][N], energy[B], length[B],
 * grid_extent[Bext][3] (in sigmas) -> x_out[B][N][7]. `side_stream` may be NULL (everything on `stream`); two events are
 * created and destroyed per call, nothing else is allocated. Saves ~20 foreign-function calls per kick: at the
 * reference's default 32^3 grid the host, not the GPU, was the limit. */
size_t chx_sc_kick_workspace_bytes(int64_t B, int64_t N, const int32_t* bins, int dtype);
int chx_sc_kick(const void* x_in, const void* charge, const void* survival, const void* energy, const void* length,
                const void* grid_extent, double mass_eV, int64_t B, int64_t Bx, int64_t Bq, int64_t Bs, int64_t Bext, int64_t N,
                const int32_t* bins, int dtype, void* x_out, void* workspace, size_t workspace_bytes, void* stream,
                void* side_stream, const void* post_map /*[BR][7][7] or NULL*/, int64_t BR);
/* A CHAIN of kicks inside one Segment.track on a tile-ordered beam (csrc/chx_sc_tiles.h; space_charge_kick.py:477-586 per kick):
 * between two kicks the particles barely move against the grid (its extent follows the beam sigmas), so the counting sort by
 * 8^3 deposit tile is done by the FIRST kick only; every kick then deposits straight from the ordered rows (LDS block per tile,
 * +1 layer handed to the neighbours through per-tile face buffers) and gathers with the potential block of each tile staged in
 * LDS; particles that left the tile of their slot are handled exactly on a slow path (float atomics / global loads), and when more
 * than 1/16 of the beam is misfiled the gather of that kick writes its rows in the new tile order (device-side decision, no host
 * synchronisation, no extra launch). B = 1 (one beam), grids as chx_sc_kick.
 *  - state: chx_sc_tile_state_bytes() bytes that live as long as the chain (header, tile starts, permutation, ordered
 *    weights / charges, row buffer, face buffers, the misfiled particles' grid); workspace: per-kick scratch, chx_sc_kick_sorted_workspace_bytes();
 *  - flags: CHX_SC_FIRST (1) x_in, charge, survival are the caller's arrays in the caller's order — sort; otherwise x_in is the
 *    x_out of the previous kick of the chain (possibly mapped through linear elements) and charge / survival are ignored;
 *    CHX_SC_LAST (2) x_out is written in the caller's particle order (else in tile order);
 *    CHX_SC_INDEX(i) (bits 8..): the kick's position in its chain, 0 for the first. With it (fp32 beams, grid edges up to 128 along
 *    x) the kicks from the second one on launch NO one-workgroup kernels: the grid geometry is formed inside the deposit and the
 *    Green function's corner-table launches from sums the previous kick's gather pass adds up with fp64 atomics, and the deposit's
 *    bookkeeping rides in the convolution's first FFT pass (csrc/chx_sc_geom_dev.h: 13 launches per kick instead of 15). The
 *    sums' last bits depend on the order of the atomics, like the charge grid's. Without an index (0) every kick launches the
 *    geometry and bookkeeping kernels. An indexed kick must not be handed beam_moments (chx_sc_kick_sorted_begin);
 *  - post_map (may be NULL): the linear run behind the kick, applied in the same particle pass (as chx_sc_kick).
 * The pieces are entry points of their own: chx_sc_beam_geometry_tiles (= chx_sc_beam_geometry + the header update),
 * chx_sc_tile_sort, chx_sc_tile_deposit (rho[gx][gy][gz], every cell stored: no zero fill), chx_sc_tile_gather_kick. */
#define CHX_SC_FIRST 1
#define CHX_SC_LAST 2
#define CHX_SC_INDEX(i) ((int)(i) << 8)
size_t chx_sc_tile_state_bytes(int64_t N, const int32_t* bins, int dtype);
size_t chx_sc_kick_sorted_workspace_bytes(int64_t N, const int32_t* bins, int dtype);
int chx_sc_kick_sorted(const void* x_in, const void* charge, const void* survival, const void* energy, const void* length,
                       const void* grid_extent, double mass_eV, int64_t N, const int32_t* bins, int dtype, void* x_out,
                       void* workspace, size_t workspace_bytes, void* state, size_t state_bytes, int flags, void* stream,
                       void* side_stream, const void* post_map);
/* chx_sc_kick_sorted in two halves, for a beam whose particles are spread over several GPUs (one process per GPU,
 * cheetah_amd/sharding.py; the reference's kick, space_charge_kick.py:477-586, needs the beam sizes of ALL particles :531-538 and
 * the charge of ALL particles on the grid :556-563): the two exchanges sit between the halves and the rows never leave the
 * tile order.
 *  begin : grid geometry — from beam_moments when non-NULL (chx_moments layout; moment_rows = 0: the 29 moments of the WHOLE
 *          beam, moment_rows = R > 0: the [R][29] moments of its shards exactly as the ranks all-gathered them, merged inside the
 *          geometry kernel with chx_merge_moments' arithmetic), else from this process's own rows as chx_sc_kick_sorted does — then
 *          [side stream: Green spectrum], [CHX_SC_FIRST: tile sort], tile deposit. *rho_out = the compact charge grid
 *          [gx][gy][gz] (dtype) inside `state` (the chain's accumulation grid): sum it over the ranks in place.
 *  finish: convolution (joins the side stream) -> gather + kick (+ post_map) into x_out.
 * Same workspace / state / flags / streams for both halves; the workspace must not be touched in between.
 * chx_sc_tile_beam_moments: this process's share of the moments the NEXT kick's grid needs — the sums the last
 * gather pass left in `state`, as a chx_moments row (entries of x, y, tau; zeros elsewhere) for the all-gather + merge. */
int chx_sc_kick_sorted_begin(const void* x_in, const void* charge, const void* survival, const void* energy, const void* length,
                             const void* grid_extent, double mass_eV, int64_t N, const int32_t* bins, int dtype, void* workspace,
                             size_t workspace_bytes, void* state, size_t state_bytes, int flags, const double* beam_moments,
                             int32_t moment_rows, void** rho_out, void* stream, void* side_stream);
int chx_sc_kick_sorted_finish(const void* x_in, const void* energy, double mass_eV, int64_t N, const int32_t* bins, int dtype,
                              void* x_out, void* workspace, size_t workspace_bytes, void* state, size_t state_bytes, int flags,
                              void* stream, void* side_stream, const void* post_map);
int chx_sc_tile_beam_moments(const void* state, size_t state_bytes, int64_t N, const int32_t* bins, int dtype, double* moments_out,
                             void* stream);
/* partials[8][nblk] (the sums of chx_sc_tile_gather_kick: W, W2, sum w x / y / tau, sum w x^2 / y^2 / tau^2 about the origin)
 * -> one chx_moments row [29] with the x, y, tau means and variances filled (statistics.py:30-48), zeros elsewhere */
int chx_sc_partials_moments(const double* partials, int64_t nblk, double* moments_out, void* stream);
/* chx_sc_geometry (B = 1 in a chain) + the header update of a chain of tile-ordered kicks (tile_header = start of the chain's
 * state for every kick but the first, NULL otherwise) */
int chx_sc_geometry_tiles(const double* moments, const void* grid_extent, const void* energy, const void* length, double mass_eV,
                          double pot_factor, int64_t B, int64_t Bm, int64_t Bext, int64_t Be, int64_t Bl, const int32_t* bins,
                          int dtype, void* half, void* cell, void* gamma, void* dt, void* scale, void* extent, double* pot_scale,
                          void* tile_header, int32_t merge_rows /*0, or B = 1 and moments[merge_rows][29] = shards to merge*/, void* stream);
int chx_sc_beam_geometry_tiles(const void* x, const void* w, const void* grid_extent, const void* energy, const void* length,
                               double mass_eV, double pot_factor, int64_t B, int64_t Bx, int64_t Bw, int64_t Bext, int64_t Be,
                               int64_t Bl, int64_t N, const int32_t* bins, int dtype, void* half, void* cell, void* gamma, void* dt,
                               void* scale, void* extent, double* pot_scale, void* workspace, size_t workspace_bytes,
                               void* tile_header, int tile_first, void* stream);
/* the geometry kernel of chx_sc_beam_geometry alone, from partial sums partials[8][nblk] (double) that chx_sc_tile_gather_kick
 * accumulated over the rows it wrote (B = 1) */
int chx_sc_geometry_from_partials(const double* partials, int64_t nblk, const void* grid_extent, const void* energy,
                                  const void* length, double mass_eV, double pot_factor, const int32_t* bins, int dtype, void* half,
                                  void* cell, void* gamma, void* dt, void* scale, void* extent, double* pot_scale, void* tile_header,
                                  void* stream);
int chx_sc_tile_sort(const void* x_in, const void* charge, const void* survival, const void* extent, const void* scale, int64_t N,
                     const int32_t* bins, int dtype, void* state, size_t state_bytes, void* stream);
/* rows: the tile-ordered rows (NULL = the state's own row buffer, which chx_sc_tile_sort filled); allow_reorder: may the crosser
 * pass order a re-sort by this kick's gather (0 for the last kick of a chain, which restores the caller's order instead). */
int chx_sc_tile_deposit(const void* rows, const void* extent, const void* scale, int64_t N, const int32_t* bins, int dtype,
                        void* state, size_t state_bytes, void* grid, int allow_reorder, void* stream);
/* chx_sc_tile_deposit with the charge LEFT in the chain's accumulation grid (*acc_out: [gx][gy][gz] of dtype inside `state`, all
 * zero between two kicks): what chx_sc_kick_sorted uses. Whoever consumes the grid must leave zeros behind —
 * chx_sc_convolve_halo_consume (= chx_sc_convolve_halo_after whose first FFT pass writes zeros behind its loads) does. */
int chx_sc_tile_deposit_acc(const void* rows, const void* extent, const void* scale, int64_t N, const int32_t* bins, int dtype,
                            void* state, size_t state_bytes, int allow_reorder, void** acc_out, void* stream);
int chx_sc_convolve_halo_consume(void* rho, const void* Ghat, const double* scale, int64_t B, const int32_t* bins, int dtype,
                                 void* phi_halo, void* workspace, size_t workspace_bytes, void* stream, void* ghat_ready_event);
int chx_sc_tile_gather_kick(const void* rows, const void* phi_halo, const void* half, const void* cell, const void* gamma,
                            const void* energy, const void* dt, double mass_eV, int64_t N, const int32_t* bins, int dtype,
                            const void* post_map, void* state, size_t state_bytes, int unpermute, void* x_out, void* stream);
/* A STRETCH of lattice — [run of skippable elements | active Cavity]+ with scalar device settings, ONE beam — in two launches:
 * what Segment.track's element-by-element walk (segment.py:545-574; cavity.py:100-251 per cavity) does with two launches and
 * ~8 us of host time per item. Launch 1 (chx_lattice_prepare, a workgroup per item): every run's composed map, every cavity's
 * map and coefficient row for the reference energy it receives (walked through the cavities in front of it), the outgoing
 * energy and path length. Launch 2: every particle through all items in registers. Bit-identical to tracking the items one by
 * one with chx_run_track / chx_cavity_track_scalars.
 *  table (device, int64 words): items[n_items][4] = {0 run | 1 cavity, elements E, first element, 0} (| 2, 3: see
 *    chx_lattice_track_diag), elem_kind[n_elems],
 *    elem_poff[n_elems] (index of the element's first pointer), ptrs[n_ptrs] (device addresses of the settings, each kind's
 *    parameters in chx_build_rmatrix order; a cavity: length, voltage, phase, frequency);
 *  state: chx_lattice_state_bytes(n_items, n_elems) bytes of device scratch that belong to the plan;
 *  energy, energy_out, s_in, s_out: one value of `dtype` each (s_in / s_out may both be NULL). */
size_t chx_lattice_state_bytes(int64_t n_items, int64_t n_elems);
int chx_lattice_prepare(const int64_t* table, int64_t n_items, int64_t n_elems, int64_t n_ptrs, const void* energy, double mass_eV,
                        double n_charges, int dtype, void* state, size_t state_bytes, void* energy_out, const void* s_in, void* s_out,
                        void* stream);
int chx_lattice_track(const int64_t* table, int64_t n_items, int64_t n_elems, int64_t n_ptrs, const void* energy, double mass_eV,
                      double n_charges, int dtype, void* state, size_t state_bytes, const void* x_in, void* x_out, int64_t N,
                      void* energy_out, const void* s_in, void* s_out, void* stream);
/* The same stretch with ACTIVE beam position monitors and apertures in it — elements that read or thin the beam and let the
 * particles pass, each of which costs the element-by-element walk (segment.py:545-574) a stop and several launches:
 *  {2, 0, q, slot}: a BPM (bpm.py:77-87): ptrs[q] = address of its misalignment [2]; readings[slot] = (dtype)(sum w x / sum w,
 *     sum w y / sum w) - misalignment of the beam AT that point (fp64 sums per wave in the particle pass, one more launch). In a big
 *     float32 scan (Bx = 1, Bm = B >= 8, B * N >= 8e6, rows on 16-byte boundaries, one row of weights) a monitor with nothing but maps
 *     and monitors in front of it is evaluated by taking the beam's weighted mean through the row's maps in fp64 instead — the same
 *     number up to the per-item float32 rounding of the individual particles, which averages out (~1e-10 of the beam size);
 *  {3, 0 rectangular | 1 elliptical, q, 0}: an aperture (aperture.py:90-135): ptrs[q], ptrs[q + 1] = addresses of x_max, y_max;
 *     survival *= inside(x, y), the arithmetic of chx_aperture_mask; monitors behind it weigh with the reduced probabilities.
 * B beams of N particles each (x_in / x_out [B][N][7]: a vectorised ParticleBeam under ONE lattice setting and energy — the same
 * maps for all beams; chx_lattice_track: B = 1). Bx = 1: x_in is ONE beam [N][7] shared by the B rows; Bm = B: the lattice
 * settings are vectorised over the rows (tagged addresses, state of chx_lattice_state_bytes_batched(.., Bm); small_runs as for
 * chx_lattice_prepare_rows): row b of the output = the beam through row b of the settings. survival: [Bw][N] (Bw = 1: one row of weights for
 * all rows), survival_out [B][N] of `dtype` or NULL (= 1); survival_out: [B][N], required when
 * the stretch holds an aperture, else NULL; readings[n_bpm][B][2]; workspace: chx_lattice_diag_workspace_bytes(N, B, n_bpm)
 * bytes. Particles, energy and path length are those of chx_lattice_track bit for bit. */
size_t chx_lattice_diag_workspace_bytes(int64_t N, int64_t B, int64_t n_bpm);
int chx_lattice_track_diag(const int64_t* table, int64_t n_items, int64_t n_elems, int64_t n_ptrs, const void* energy, double mass_eV,
                           double n_charges, int dtype, void* state, size_t state_bytes, const void* x_in, void* x_out, int64_t N,
                           int64_t B, int64_t Bx, int64_t Bm, int64_t Bw, int small_runs, void* energy_out, const void* s_in,
                           void* s_out, const void* survival, void* survival_out, int64_t n_bpm, void* readings, void* workspace,
                           size_t workspace_bytes, void* stream);
/* The same stretch with ACTIVE SCREENS in it (screen.py:187-239: the screen records a copy of the beam that reaches it and lets
 * the beam pass; screen.py:241-344: its image). An RL control step is `Segment.track` on a small beam followed by the screen's
 * reading: element by element that is the merged track, a copy of five tensors, a memset and the deposit — four launches and
 * ~50 us of host time around ~10 us of work. Here the screen is an item of the stretch:
 *  {4, flags, q, slot}: ptrs[q] = address of its misalignment [2], ptrs[q + 1] = address of its pixel_size [2] (both `dtype`),
 *     ptrs[q + 2 .. q + 5] = the integers resolution_x, resolution_y, bins_x, bins_y (bins = resolution // binning);
 *     flags bit 0: deposit the cloud-in-cell image (screen.py:327-339) in the particle pass.
 * screens[slot] (HOST array, read before the call returns) holds this call's output buffers of the screen:
 *  rows [N][7], charges [N], survival [N]: the record of the beam AT the screen (the coordinates UNSHIFTED: the misalignment is
 *     subtracted where the image is formed and by the caller's `get_read_beam`), written by the particle pass; each may be NULL;
 *  energy, s: one value of `dtype` each — the reference energy and path length at the screen, written by the preparation launch;
 *  image [bins_y][bins_x] (`dtype`; NULL = none) of image_bytes bytes: ZEROED by the preparation launch (spare workgroups: no
 *     memset launch), then every particle adds |charge| * survival to its four pixels with the index arithmetic of
 *     chx_cic_deposit on (x - misalignment_x, y - misalignment_y) and the extent (-+ resolution * pixel_size / 2) evaluated from
 *     the pixel size as torch evaluates screen.py:139-148 — the same cells, fractions and addends as
 *     chx_apply_affine7 + chx_cic_deposit on the recorded rows (float atomics: the same sum to the order of the additions);
 *  ParameterBeam variant (chx_parameter_lattice_track_screens): mu [7], cov [49] = the moments at the screen; image
 *     [height][width] = chx_screen_gaussian of them (geom: [left, hstep, bottom, vstep], shift: the misalignment; one more launch).
 * One beam, scalar settings (B = Bx = Bm = Bw = 1) when n_screens > 0; `charge` [N] (may be NULL = 1) feeds the image weights
 * and the record. */
#define CHX_LATTICE_MAX_SCREENS 4
typedef struct chx_lattice_screen {
    void* rows;
    void* charges;
    void* survival;
    void* energy;
    void* s;
    void* image;
    int64_t image_bytes;
    void* map;              /* [7][7] (`dtype`) or NULL: the composed map of the RUN right in front of the screen, as the particle
                               pass applies it (what a differentiable caller hangs the screen's beam properties on) */
    void* element_maps;     /* [E][7][7] (`dtype`) or NULL: that run's element maps in tracking order (what chx_run_vjp_masked takes) */
    /* ParameterBeam variant only */
    void* mu;
    void* cov;
    const void* geom;
    const void* shift;      /* the screen's misalignment [2] (`dtype`, device) */
    const void* total_charge; /* the beam's total charge (one value of `dtype`) and where the record's copy of it goes */
    void* total_charge_out;
    int32_t width, height;
    /* ParticleBeam variant, round 6 (ABI 8): the particle pass also adds the one-pass sums of the recorded beam's 29 moments
     * (particle_beam.py:1699-1717; utils/statistics.py:4-62) — about the beam's first row as it stands at the screen — into
     * mom_partials: CHX_LATTICE_MOMENT_DOUBLES doubles = n sets (n = chx_lattice_moment_blocks(N, B) <= 64) of {W, W2, s[6], m[21]} as
     * [29][n], the centre[6] behind them; the preparation launch zeroes the buffer — or NULL. chx_lattice_screen_moments
     * adds the sets and finalises: a beam property of the screen's beam costs one small launch, no pass over its rows.
     * Not together with `image` in one call. */
    void* mom_partials;
} chx_lattice_screen;
#define CHX_LATTICE_MOMENT_DOUBLES (29 * 64 + 6)
/* the sets of partial sums the particle pass of chx_lattice_track_screens uses for N particles x B beams (at most 64 per beam) */
int64_t chx_lattice_moment_blocks(int64_t N, int64_t B);
/* mom_partials (n_blocks = chx_lattice_moment_blocks sets) -> out[29] = {W, W2, mu[6], cov[21]} (what chx_moments gives for the
 * recorded rows, to the rounding of another summation order) and, index >= 0, entry_out[1] (`dtype`) = out[index] or its square
 * root (chx_moments_entry). */
int chx_lattice_screen_moments(const double* mom_partials, int64_t n_blocks, int dtype, double* out, int index, int take_sqrt,
                               void* entry_out, void* stream);
/* (ABI 9: B > 1 beams with screens when Bm == 1 — records [B][N][7] / [B][N] / [B][N], images [B][height][width], `charge` one row of N
 * shared by the beams; mom_partials only with B == 1.) */
int chx_lattice_track_screens(const int64_t* table, int64_t n_items, int64_t n_elems, int64_t n_ptrs, const void* energy,
                              double mass_eV, double n_charges, int dtype, void* state, size_t state_bytes, const void* x_in,
                              void* x_out, int64_t N, int64_t B, int64_t Bx, int64_t Bm, int64_t Bw, int small_runs,
                              void* energy_out, const void* s_in, void* s_out, const void* survival, void* survival_out,
                              int64_t n_bpm, void* readings, void* workspace, size_t workspace_bytes, const void* charge,
                              const chx_lattice_screen* screens, int64_t n_screens, void* stream);
/* A stretch's table (the `table` argument of the chx_lattice_* calls: device memory) written from HOST words without a staging
 * buffer — the words travel in the arguments of a one-workgroup launch on `stream`, in front of the preparation launch that reads
 * them: n <= chx_table_store_max_words(). For a host whose control loop assigns new setting tensors every step (README.md:73-77):
 * the table's layout stands, a few addresses change. */
int64_t chx_table_store_max_words(void);
int chx_table_store(const int64_t* host_words, int64_t n, void* table, void* stream);
/* chx_lattice_prepare_rows that also writes screens[slot].energy / .s and zeroes screens[slot].image (rows = 1 when n_screens > 0) */
int chx_lattice_prepare_screens(const int64_t* table, int64_t n_items, int64_t n_elems, int64_t n_ptrs, int64_t rows, int small_runs,
                                const void* energy, double mass_eV, double n_charges, int dtype, void* state, size_t state_bytes,
                                void* energy_out, const void* s_in, void* s_out, const chx_lattice_screen* screens,
                                int64_t n_screens, void* stream);
/* out[4] (`dtype`, device) = the extent (left, right, bottom, top) the stretch kernels derive from pixel_size[2] (`dtype`, device)
 * and the resolution — for checking it bit for bit against the reference's tensor expression (screen.py:139-148) */
int chx_screen_extent(const void* pixel_size, int32_t resolution_x, int32_t resolution_y, int dtype, void* out, void* stream);
/* The same stretch for a ParameterBeam (element.py:167-179, cavity.py:127-133,202-218, bpm.py:77-87): mu [Bmu][7], cov [Bcov][49]
 * (Bmu, Bcov in {1, B}) through [run | active Cavity | active BPM]+ by one wavefront per batch row after the same preparation
 * launch — mu' = R mu, cov' = R cov R^T item by item (fp64 inside, rounded to `dtype` between items like chx_parameter_track), a
 * cavity's moment updates, readings[n_bpm][B][2] = (mu_x, mu_y) - misalignment at every monitor. Items of type 3 are skipped. */
/* Bm = rows of lattice settings (1, or B: the settings are vectorised — ptrs entries with the lowest bit set address (B,) arrays of
 * `dtype`, like chx_run_map_batched; lengths, cavity settings and the energy stay scalars): row b of the beam goes through row b of
 * the lattice; state: chx_lattice_state_bytes_batched(n_items, n_elems, Bm) bytes (chx_lattice_prepare_batched fills it). */
size_t chx_lattice_state_bytes_batched(int64_t n_items, int64_t n_elems, int64_t rows);
int chx_lattice_prepare_batched(const int64_t* table, int64_t n_items, int64_t n_elems, int64_t n_ptrs, int64_t rows, const void* energy,
                                double mass_eV, double n_charges, int dtype, void* state, size_t state_bytes, void* energy_out,
                                const void* s_in, void* s_out, void* stream);
/* small_runs is a set of flags. Bit 0 (CHX_LATTICE_SMALL_RUNS): the caller vouches that the stretch holds no cavity and no run of
 * more than 64 elements — a wave per (item, row) prepares the maps instead of a workgroup (300 000 of them for 75 items x 4096
 * rows); the same results. Bit 1 (CHX_LATTICE_ENERGY_ROWS): `energy` and `energy_out` are (rows,) arrays — a scan of BEAM ENERGIES,
 * row r of the maps, coefficient rows and outgoing energies belongs to energy r (cavity.py:113-122 per row; the second-order
 * path-length switch of cavity.py:157 depends on the cavity's settings only, which are scalars here). The same flags travel through
 * the `small_runs` argument of chx_lattice_track_diag and chx_parameter_lattice_track. Bit 2 (CHX_LATTICE_ENERGY_OUT_ROWS):
 * `energy_out` alone is a (rows,) array — a cavity whose voltage or phase is vectorised (tagged addresses) hands on one energy per
 * row; cavity.py:157's `(delta_energy > 0).any()` is then taken over the rows of that cavity. */
#define CHX_LATTICE_SMALL_RUNS 1
#define CHX_LATTICE_ENERGY_ROWS 2
#define CHX_LATTICE_ENERGY_OUT_ROWS 4
/* bit 3: the caller vouches that every run holds at most 64 elements (cavities allowed): with rows > 1 a wave per (item, row) prepares
 * the stretch, cavity arithmetic included (a 16-cell linac at 64 energies: 2048 workgroups of four waves otherwise) */
#define CHX_LATTICE_SHORT_RUNS 8
int chx_lattice_prepare_rows(const int64_t* table, int64_t n_items, int64_t n_elems, int64_t n_ptrs, int64_t rows, int small_runs,
                             const void* energy, double mass_eV, double n_charges, int dtype, void* state, size_t state_bytes,
                             void* energy_out, const void* s_in, void* s_out, void* stream);
int chx_parameter_lattice_track(const int64_t* table, int64_t n_items, int64_t n_elems, int64_t n_ptrs, const void* energy,
                                double mass_eV, double n_charges, int dtype, void* state, size_t state_bytes, const void* mu,
                                const void* cov, int64_t B, int64_t Bmu, int64_t Bcov, int64_t Bm, int small_runs, void* mu_out,
                                void* cov_out, void* energy_out, const void* s_in, void* s_out, int64_t n_bpm, void* readings,
                                void* stream);
int chx_parameter_lattice_track_screens(const int64_t* table, int64_t n_items, int64_t n_elems, int64_t n_ptrs, const void* energy,
                                        double mass_eV, double n_charges, int dtype, void* state, size_t state_bytes, const void* mu,
                                        const void* cov, int64_t B, int64_t Bmu, int64_t Bcov, int64_t Bm, int small_runs, void* mu_out,
                                        void* cov_out, void* energy_out, const void* s_in, void* s_out, int64_t n_bpm, void* readings,
                                        const chx_lattice_screen* screens, int64_t n_screens, void* stream);
/* Cavity.track (cavity.py:100-251) for ONE beam and a cavity whose four settings are device scalars of `dtype`:
 * param_ptrs[4] = device pointers to length, voltage, phase [deg], frequency; energy = device pointer to one value;
 * kind = CHX_CAVITY_SW / CHX_CAVITY_TW. chx_cavity_prepare_scalars writes the map R_out[7][7] (dtype, as chx_build_rmatrix),
 * the coefficient row coeffs[CHX_CAV_NCOEF] (as chx_cavity_coeffs) and the outgoing energy with one thread of one launch;
 * chx_cavity_track_scalars adds the particle pass of chx_cavity_track: the whole element in one call, two launches,
 * bit-identical to chx_build_rmatrix + chx_cavity_coeffs + chx_cavity_track. */
int chx_cavity_prepare_scalars(const void* const* param_ptrs, const void* energy, int kind, double mass_eV, double n_charges,
                               int dtype, void* R_out, double* coeffs, void* energy_out, const void* s_in /*may be NULL*/,
                               void* s_out /*NULL iff s_in is: *s_out = *s_in + length*/, void* stream);
size_t chx_cavity_track_scalars_workspace_bytes(void);
int chx_cavity_track_scalars(const void* x_in, const void* const* param_ptrs, const void* energy, int kind, double mass_eV,
                             double n_charges, int64_t N, int dtype, void* x_out, void* energy_out, const void* s_in,
                             void* s_out, void* workspace, size_t workspace_bytes, void* stream);
/* n <= 8 device arrays copied by one launch: dst[k][0 .. bytes[k]) = src[k][...] (host arrays of device pointers and byte
 * counts). What a Screen's record of the incoming beam costs (screen.py:190 `incoming.clone()`: five tensors). */
int chx_copy_arrays(const void* const* src, void* const* dst, const int64_t* bytes, int32_t n, void* stream);
/* SI conversion on its own (particle_beam.py:1262-1346), used by to_xyz_pxpypz/from_xyz_pxpypz */
int chx_to_xyz_pxpypz(const void* x_in, const void* energy, double mass_eV, int64_t B, int64_t Bx,
                      int64_t Be, int64_t N, int dtype, void* xp_out, void* stream);
int chx_from_xyz_pxpypz(const void* xp_in, const void* energy, double mass_eV, int64_t B,
                        int64_t Bx, int64_t Be, int64_t N, int dtype, void* x_out, void* stream);

/* ---- ParameterBeam path (element.py:167-179, cavity.py:127-133,202-218,
 * screen.py:255-291). mu[Bmu][7], cov[Bcov][7][7], R[BR][7][7]: mu' = R mu, cov' = R cov R^T (fp64 inside).
 * With cavity_coeffs (double [B][CHX_CAV_NCOEF] from chx_cavity_coeffs) the reference's cavity moment
 * updates are applied on top (mu_tau, mu_delta, cov_tautau, cov_taudelta, cov_deltadelta). */
int chx_parameter_track(const void* mu, const void* cov, const void* R, const double* cavity_coeffs, int64_t B,
                        int64_t Bmu, int64_t Bcov, int64_t BR, int dtype, void* mu_out, void* cov_out,
                        void* stream);
/* Backward of the linear part (no cavity coefficients): g_mu[B][7], g_cov[B][7][7] (dtype; either may be NULL = zero) ->
 * d_mu[B][7] = R^T g, d_cov[B][7][7] = R^T G R, d_R[B][7][7] = g mu^T + G R cov^T + G^T R cov, one row per batch row (the
 * caller sums the rows of a broadcast input); each output may be NULL. What autograd derives from element.py:167-179
 * (tests/test_differentiable.py:58-75). */
int chx_parameter_track_bwd(const void* g_mu, const void* g_cov, const void* mu, const void* cov, const void* R, int64_t B,
                            int64_t Bmu, int64_t Bcov, int64_t BR, int dtype, void* d_mu, void* d_cov, void* d_R,
                            void* stream);
/* Screen reading of a ParameterBeam: bivariate normal density of (x - shift_x, y - shift_y) sampled at
 * (left + ix*hstep, bottom + iy*vstep); geom = [left, hstep, bottom, vstep] (dtype, device);
 * positions_fp32 != 0 rounds the sample positions to fp32 (the reference's torch.arange grid is created in
 * torch's default dtype, screen.py:284-287); image[B][height][width]. */
int chx_screen_gaussian(const void* mu, const void* cov, const void* shift, const void* geom, int64_t B,
                        int64_t Bmu, int64_t Bcov, int64_t Bsh, int32_t width, int32_t height,
                        int positions_fp32, int dtype, void* image, void* stream);

/* ---- non-linear per-particle tracking.
 * Drift-kick-drift (Bmad-X) tracking: drift.py:106-154, quadrupole.py:168-251, dipole.py:183-370,
 * transverse_deflecting_cavity.py:122-209 over utils/bmadx.py. Cheetah -> Bmad canonical coordinates,
 * the element's exact/symplectic map, and back, in one pass; column 6 of x_out is 1.
 * params[Bp][P] (dtype):
 *   CHX_DKD_DRIFT       [length]
 *   CHX_DKD_QUADRUPOLE  [length, k1, tilt, misalignment_x, misalignment_y]   (+ num_steps)
 *   CHX_DKD_DIPOLE      [length, angle, e1, e2, tilt, fint, fint_exit, gap, gap_exit]
 *                       (+ fringe_at: bit 0 = entrance, bit 1 = exit; linear_edge fringe)
 *   CHX_DKD_TDC         [length, voltage, phase, frequency, tilt, misalignment_x, misalignment_y]
 *   CHX_DKD_SEXTUPOLE   [length, k2, tilt, misalignment_x, misalignment_y]   (+ num_steps = n, 1 <= n < 2^25)
 *                       Bmad's exact drifts around thin kicks (the reference has no such method for its Sextupole; the building
 *                       blocks are its bmadx.track_a_drift and offset_particle_set / _unset): with h = L / (2 n), kappa = k2 L / n:
 *                       offset_set, drift(h), n x { px -= (kappa / 2)(x^2 - y^2), py += kappa x y, drift(2 h; h after the last
 *                       kick) }, offset_unset — n kicks, n + 1 drifts, pz unchanged, symplectic; k2 = 0: a drift of length L.
 *   CHX_DKD_RFCAVITY    [length, voltage, phase, frequency]   (num_steps and fringe_at are not read; length = 0: a thin cavity)
 *                       Bmad's rfcavity (bmad_standard) from the same building blocks: drift(L / 2); with the particle's time
 *                       offset t = -z / (beta c) the energy kick dE = |n_charges| voltage sin(2 pi (phase - frequency t)), E' = E + dE,
 *                       pc' = sqrt(E'^2 - m^2), pz += dE (2 E + dE) / ((pc' + pc) p0c) (= (pc' - pc) / p0c without the cancellation;
 *                       dE = 0 leaves pz as it is), z *= beta' / beta; drift(L / 2). phase in units of 2 pi; frequency t is reduced in turns (u - rint(u))
 *                       before the sine, and sin, cos of 2 pi phase are taken once per element, so phase = 0 and 0.5 are exact zero
 *                       crossings. x, px, y, py see only the drifts: symplectic. The reference energy is NOT changed (the
 *                       storage-ring convention); total energy below the rest mass behind the kick: NaN.
 *   CHX_DKD_MULTIPOLE   [length, knl, ksl, tilt, misalignment_x, misalignment_y]   (+ num_steps = n, 1 <= n < 2^25; fringe_at = the
 *                       order m = 0 .. 3 of the kick: 0 dipole, 1 quadrupole, 2 sextupole, 3 octupole; length = 0: a thin element)
 *                       The Sextupole's frame with the kick of one order: knl, ksl are the INTEGRATED normal and skew strengths
 *                       in m^-m (MAD-X's knl / ksl). With h = L / (2 n): offset_set, drift(h), n x { d px - i d py =
 *                       -(knl + i ksl) / n (x + i y)^m / m!, drift(2 h; h after the last kick) }, offset_unset. (x + i y)^m by m
 *                       complex multiplications from 1, 1 / m! folded into the strengths once per element: the backward pass has
 *                       the right derivative at x = y = 0 and at knl = ksl = 0. pz unchanged, symplectic; knl = ksl = 0: a drift
 *                       of length L; m = 2, ksl = 0: CHX_DKD_SEXTUPOLE with k2 = knl / L; m = 0: d px = -knl, d py = +ksl.
 * fringe_at: the Dipole's fringe bits; for CHX_DKD_MULTIPOLE: the order m. No other kind reads it.
 * energy_out[B] (may be NULL) receives the reference energy recomputed from p0c (bmadx.py:49). */
enum chx_dkd_kind { CHX_DKD_DRIFT = 0, CHX_DKD_QUADRUPOLE = 1, CHX_DKD_DIPOLE = 2, CHX_DKD_TDC = 3,
                    CHX_DKD_LINEAR = 4 /* only in chx_dkd_chain_mixed / chx_dkd_energy_chain: a merged run of linear elements */,
                    CHX_DKD_SEXTUPOLE = 5, CHX_DKD_RFCAVITY = 6, CHX_DKD_MULTIPOLE = 8 /* (7 is no kind) */ };
/* The parameter count of a kind, -1 for anything else — and, still, for CHX_DKD_RFCAVITY and CHX_DKD_MULTIPOLE: the kinds came
 * without a change of the ABI version, and a caller of ABI 9 that probes the kinds with this function sees the set it knew. Their
 * counts are 4 and 6 (above); chx_dkd_bwd_partials_count and every entry point that takes a kind count them. */
int chx_dkd_num_params(int kind);
int chx_dkd_track(int kind, const void* x_in, const void* params, const void* energy, double mass_eV,
                  double n_charges, int32_t num_steps, int32_t fringe_at, int64_t B, int64_t Bx, int64_t Bp,
                  int64_t Be, int64_t N, int dtype, void* x_out, void* energy_out, void* stream);
/* The same with the arithmetic width as an argument: storage_precision = 0 evaluates the per-particle map in float64 whatever
 * the storage dtype (chx_dkd_track: agreement with Bmad-X to 1e-14 in float64, ~1e-7 of a coordinate in float32, but fp64-VALU
 * bound: 20-42 us per element at 1e6 particles); 1 evaluates float32 beams in float32 like the reference's own tensor code
 * (cheetah/utils/bmadx.py runs in the beam dtype) — one HBM-bound pass. float64 beams ignore the flag. */
int chx_dkd_track_p(int kind, const void* x_in, const void* params, const void* energy, double mass_eV, double n_charges,
                    int32_t num_steps, int32_t fringe_at, int64_t B, int64_t Bx, int64_t Bp, int64_t Be, int64_t N, int dtype,
                    int storage_precision, void* x_out, void* energy_out, void* stream);
/* A run of E drift-kick-drift elements (a lattice tracked with tracking_method = "drift_kick_drift": every element is its own,
 * non-mergeable map, e.g. quadrupole.py:174-240) on one beam x_in[N][7] with scalar settings: HOST arrays kinds[E],
 * params[E] (device pointers to each element's parameter array), num_steps[E], fringe_at[E], storage_precision[E]; the
 * reference energy travels from element to element on the device (energies[E] (dtype): what each element leaves; energy_in one
 * scalar). x_tmp[N][7] is scratch (may be NULL for E = 1); x_out receives the last element's particles. Drifts, Quadrupoles,
 * Dipoles, Sextupoles, RFCavities and Multipoles (float32 beams: of one storage_precision): two launches per 320 elements, the particles in registers across the run (x_tmp
 * holds the elements' constants); otherwise E launches. Either way one call and the bits of E separate chx_dkd_track_p calls.
 * s_in / s_out (one scalar of dtype each, both or neither): the path length, s_out = (((s_in + l_0) + l_1) + ...) with the
 * lengths added one by one in dtype like the reference's `s=incoming.s + self.length` per element. */
int chx_dkd_chain(const int32_t* kinds, const void* const* params, const int32_t* num_steps, const int32_t* fringe_at,
                  const int32_t* storage_precision, int64_t E, const void* x_in, const void* energy_in, double mass_eV,
                  double n_charges, int64_t N, int dtype, void* x_out, void* x_tmp, void* energies, const void* s_in, void* s_out,
                  void* stream);
/* The same run with merged runs of linear elements in between (a lattice whose drifts are tracked linearly and whose magnets with
 * the Bmad-X maps; segment.py:545-574 tracks such a run with its composed map): kinds[e] = CHX_DKD_LINEAR marks params[e] as a
 * [7][7] first-order map (dtype), applied with the arithmetic of chx_apply_affine7, and lengths[e] as the device scalar holding
 * that run's summed length (lengths may be NULL when no item is linear; the entry of a drift-kick-drift element may be NULL: its
 * first parameter). The reference energy passes a linear run unchanged. One pass over the beam for the whole stretch. */
int chx_dkd_chain_mixed(const int32_t* kinds, const void* const* params, const void* const* lengths, const int32_t* num_steps,
                        const int32_t* fringe_at, const int32_t* storage_precision, int64_t E, const void* x_in, const void* energy_in,
                        double mass_eV, double n_charges, int64_t N, int dtype, void* x_out, void* x_tmp, void* energies,
                        const void* s_in, void* s_out, void* stream);
/* energies[E] (dtype) = the reference energy behind every item of such a run without tracking anything (a caller that builds the
 * maps of the linear runs needs the energy in front of each of them). kinds_scratch: E int32 of device memory. One or two launches. */
int chx_dkd_energy_chain(const int32_t* kinds, int64_t E, const void* energy_in, double mass_eV, int dtype, void* energies,
                         void* kinds_scratch, void* stream);
/* A ring of E drift-kick-drift Drifts, Quadrupoles, Dipoles, Sextupoles, RFCavities and Multipoles (the symplectic Bmad-X maps) turn after turn: turns [first_turn,
 * first_turn + num_turns) in one particle launch, the particles in registers from turn to turn; the bits of num_turns passes of
 * chx_dkd_chain. HOST arrays kinds[E] (CHX_DKD_DRIFT / _QUADRUPOLE / _DIPOLE / _SEXTUPOLE / _RFCAVITY / _MULTIPOLE), params[E], num_steps[E], fringe_at[E] as in
 * chx_dkd_chain, 1 <= E <= 192; ONE storage_precision (0 double, 1 storage, 2 mixed) for the ring, ignored by float64 beams.
 *   energy_in (dtype scalar): the reference energy in front of turn first_turn; energy_out: the energy behind the last turn of the
 *     call (may be energy_in: the chunks of a call hand it on through one device scalar). Every element leaves the round trip
 *     sqrt(sqrt(E^2 - m^2)^2 + m^2) of the energy it received, which need not be a fixed point: the call walks the energy through its
 *     turns on the device and computes one block of element constants per turn until two turns in a row start with the same
 *     energy bits — from there on the turns share a block. Exact for every energy.
 *   lost_turn, aperture, charges, survival, record_every, sums[record][14], probe[record][K][7], the aliasing of x_in / x_out and
 *     s_in / s_out (the path length after ONE turn): as in chx_second_order_turns.
 *   workspace: chx_dkd_turns_workspace_bytes(E, N, turns of this call, records of this call, dtype) bytes, 16-byte aligned — the
 *     turns' start energies (dtype), block_of_turn[turns + 1] (int32), turns x E x 56 doubles of constants (the worst case: the
 *     host cannot know how many blocks the device opens) and records x ceil(N / 256) x 14 doubles of partial sums; the first two
 *     parts rounded up to 16 bytes. The function is monotone in every argument and returns 0 for arguments out of range.
 * Four launches (energy walk, constants and path length, particles, reduction of the records), none synchronising.
 * CHX_ERR_INVALID_ARG, before any launch: E < 1, E > 192, a kind other than the six, storage_precision outside 0..2, num_steps
 * outside 1 .. 2^25 - 1, fringe_at outside 0..3, num_turns < 1, record_every < 1, K > N, a last turn of 2^31 - 1 or beyond, aliased
 * buffers, a workspace too small or not 16-byte aligned, a required pointer that is NULL; CHX_ERR_DTYPE: dtype other than CHX_F32
 * / CHX_F64. */
size_t chx_dkd_turns_workspace_bytes(int64_t E, int64_t N, int64_t turns_in_chunk, int64_t records_in_chunk, int dtype);
int chx_dkd_turns(const int32_t* kinds, const void* const* params, const int32_t* num_steps, const int32_t* fringe_at,
                  int storage_precision, int64_t E, const void* x_in, const void* energy_in, void* energy_out, double mass_eV,
                  double n_charges, const void* charges, const void* survival, int64_t N, int dtype, int64_t first_turn,
                  int64_t num_turns, int64_t record_every, const void* aperture, int64_t K, void* x_out, int32_t* lost_turn,
                  double* sums, void* probe, const void* s_in, void* s_out, void* workspace, size_t workspace_bytes, void* stream);
/* The one-turn map of such a ring with its 6 x 6 Jacobian, and the closed orbit (Segment.one_turn_map, closed_orbit, ring_optics).
 * HOST arrays kinds[E], params[E], num_steps[E], fringe_at[E] as in chx_dkd_turns, 1 <= E <= 192, scalar settings of `dtype`;
 * energy_in (dtype scalar) is the reference energy in front of the turn, walked through ONE turn as the first turn of
 * chx_dkd_turns walks it (the same kernel prepares the same 56 doubles per item). The maps are evaluated in float64 through their
 * dual-number instantiation whatever dtype is: the values are those of storage_precision = 0, every output is float64.
 *   start[B][6]: the seeds (x, px, y, py, tau, delta).
 *   mode 0: the map at the seeds. mode 1: the 4-D closed orbit, x, px, y, py closed while tau and delta keep the seed's values.
 *     mode 2: the 6-D closed orbit (all six closed; meaningful with an RFCavity on a harmonic of the revolution frequency).
 *   num_iterations (modes 1, 2; not read in mode 0): Newton steps x_c += solve((M_c - I) step = -(f(x) - x)_c) on the closed
 *     coordinates c, by Gaussian elimination with partial pivoting in float64 on the device, followed by one more pass from the
 *     final point. A FIXED count for every seed: no early exit, two calls give the same bits. A singular or non-finite system
 *     leaves NaN in that seed's outputs and in no other's, and so does an image that is not finite (a seed beyond the dynamic
 *     aperture): orbit, image, matrix, residual and dispersion of that seed are then NaN throughout (mode 0 hands the seed back
 *     in orbit), the records along the ring stay what the last pass met.
 *   orbit[B][6]: the point the last pass started from (mode 0: the seed); image[B][6]: where it went; matrix[B][6][6], matrix[i][m] =
 *     d image_i / d orbit_m; residual[B] = max |image - orbit| over c (mode 0: over x, px, y, py); dispersion[B][4] = the solution of
 *     (I - M_4) eta = matrix[:4][5] from the same solver, in every mode (NaN when I - M_4 is singular).
 *   record_along = 1: orbit_along[B][E + 1][6] and matrix_along[B][E + 1][6][6] of the last pass — index 0 the start (the identity),
 *     index k behind item k, the cumulative map from the start — and s_along[E + 1] (dtype): 0 and the lengths added item by item
 *     in dtype as chx_dkd_chain adds them. With record_along = 0 the three pointers are not read.
 *   workspace: chx_dkd_ring_jacobian_workspace_bytes(E) bytes, 16-byte aligned (the constants and the energies behind the items);
 *     0 for E out of range.
 * One lane per (seed, tangent direction), eight lanes per seed, eight seeds per single-wave workgroup. Two launches, none
 * synchronising; the results of a seed do not depend on B.
 * CHX_ERR_INVALID_ARG, before any launch: E < 1, E > 192, a kind other than the six, num_steps outside 1 .. 2^25 - 1, fringe_at
 * outside 0..3, B < 1, mode outside 0..2, num_iterations < 1 in modes 1 and 2, record_along outside 0..1, a required pointer that is
 * NULL, a workspace too small or not 16-byte aligned; CHX_ERR_DTYPE: dtype other than CHX_F32 / CHX_F64.
 * (An additive export: CHX_ABI_VERSION stays as it is.) */
size_t chx_dkd_ring_jacobian_workspace_bytes(int64_t E);
int chx_dkd_ring_jacobian(const int32_t* kinds, const void* const* params, const int32_t* num_steps, const int32_t* fringe_at,
                          int64_t E, const void* energy_in, double mass_eV, double n_charges, int dtype, const double* start,
                          int64_t B, int mode, int64_t num_iterations, int record_along, double* orbit, double* image,
                          double* matrix, double* residual, double* dispersion, double* orbit_along, double* matrix_along,
                          void* s_along, void* workspace, size_t workspace_bytes, void* stream);
/* The derivative of chx_dkd_ring_jacobian's results with respect to K knobs on the ring's settings (Segment.ring_sensitivity,
 * the `wrt` argument of Segment.ring_optics). The ring's HOST arrays, energy_in, mass_eV, n_charges, dtype and mode as above.
 *   orbit[B][6]: the CONVERGED orbits of a chx_dkd_ring_jacobian call of the same mode (mode 0: its seeds), not guesses.
 *   A knob is a direction in the ring's flat space of parameters, given by components: HOST arrays knob_of, item_of, slot_of
 *     [num_components], component c moves parameter slot_of[c] of item item_of[c] with weight 1 as part of knob knob_of[c]. One
 *     setting shared by many items is one knob with many components. A knob without a component has zero derivatives.
 *   d_orbit[B][K][6] = d orbit / d knob (zero in mode 0 and on the held coordinates of mode 1), d_image[B][K][6] = d image / d knob,
 *     d_matrix[B][K][6][6] = d matrix / d knob: TOTAL derivatives, in modes 1 and 2 the orbit moves with the knob,
 *     (I - M_c) d orbit_c = (d f / d knob)_c by the solver of the Newton step. d_dispersion[B][K][4] = d dispersion / d knob, the
 *     solution of (I - M_4) d eta = d matrix[:4][5] + d matrix[:4][:4] eta.
 *   record_along = 1: d_orbit_along[B][K][E + 1][6] and d_matrix_along[B][K][E + 1][6][6], the derivatives of orbit_along and
 *     matrix_along (index 0: d orbit and zeros). With record_along = 0 the two pointers are not read.
 *   workspace: chx_dkd_ring_sensitivity_workspace_bytes(E, K) bytes, 16-byte aligned (the constants of a turn and their tangents,
 *     17 doubles per knob and item); 0 for E or K out of range (K <= 2^20).
 * The maps are evaluated in second-order dual numbers (csrc/chx_dual2.h): eight lanes per (seed, knob), lane m carrying the phase-
 * space direction e_m, every lane the knob; pass 1 gives d f / d knob and M, pass 2 (modes 1, 2) runs with the orbit's derivative.
 * A fixed number of passes, no atomics: two calls give the same bits, a (seed, knob)'s rows do not depend on B or K. A seed whose
 * orbit or image is not finite, or whose system is singular, is NaN in all its own rows and in no other's. K = 0 launches nothing.
 * CHX_ERR_INVALID_ARG, before any launch: the ring's conditions above, B < 1, K < 0, mode outside 0..2, record_along outside 0..1,
 * num_components < 0, a knob, item or slot out of range (slot < the item's parameter count), a component named twice, a
 * required pointer that is NULL, a workspace too small or not 16-byte aligned; CHX_ERR_DTYPE: dtype other than CHX_F32 / CHX_F64.
 * (An additive export: CHX_ABI_VERSION stays as it is.) */
size_t chx_dkd_ring_sensitivity_workspace_bytes(int64_t E, int64_t K);
int chx_dkd_ring_sensitivity(const int32_t* kinds, const void* const* params, const int32_t* num_steps, const int32_t* fringe_at,
                             int64_t E, const void* energy_in, double mass_eV, double n_charges, int dtype, const double* orbit,
                             int64_t B, int mode, const int32_t* knob_of, const int32_t* item_of, const int32_t* slot_of,
                             int64_t num_components, int64_t K, int record_along, double* d_orbit, double* d_image,
                             double* d_matrix, double* d_dispersion, double* d_orbit_along, double* d_matrix_along, void* workspace,
                             size_t workspace_bytes, void* stream);
/* The synchrotron-radiation integrals I1 .. I5 of such a ring on closed orbits chx_dkd_ring_jacobian found
 * (Segment.radiation_integrals). The ring's HOST arrays, energy_in, mass_eV, n_charges and dtype as in chx_dkd_ring_jacobian.
 *   orbit[B][6]: the CONVERGED orbits (mode 1), beta0[B][2], alpha0[B][2]: the periodic projected functions of the diagonal 2 x 2
 *     blocks of the one-turn matrix at the start of the ring, eta0[B][4]: its dispersion (chx_dkd_ring_jacobian's).
 *   integrals[B][7] = (I1, I2, I3, I4x, I4y, I5x, I5y); along[B][E][7] (may be NULL): every item's contribution, exact zeros for
 *     items that are no Dipoles. The totals are the sums over the items in their order, with and without `along`.
 * Only Dipoles contribute (one with L = 0 or angle = 0: zeros). Out of scope: feed-down in quadrupoles on an off-axis orbit,
 * order-0 Multipoles, a Dipole's k1 (the drift-kick-drift Dipole does not track it). For a Dipole with h = angle / L, tilt t:
 *   a point s = f L inside the body, 0 < f < 1: the map from the item's entrance to s rotates by the tilt, applies the entrance
 *     fringe kick if its fringe_at bit is set, the exact body map of length f L and angle f angle at the same h, and rotates back
 *     (no exit fringe). A(s) is the 6 x 6 Jacobian from the ring's start to s on the closed orbit.
 *   eta(s) = beta_rel (A[:4][:4] eta0 + A[:4][5]), beta_rel = p0c / E0: delta is dE / p0c here, the integrals are defined on
 *     d x / d (dp / p); eta' is d px / d delta (canonical). beta_u(s), alpha_u(s): the diagonal 2 x 2 block of A(s) applied to beta0_u,
 *     alpha0_u (the projected functions; a plane without a periodic solution is NaN in its I5 only).
 *     H_u = (eta_u^2 + (beta_u eta_u' + alpha_u eta_u)^2) / beta_u.
 *   I2 = L h^2 and I3 = L |h|^3 directly; with sum_j the 8-point Gauss-Legendre rule on f in (0, 1) and eta_b = eta_x cos t + eta_y sin t:
 *     I1 = L h sum_j w_j eta_b(s_j)
 *     I4x = L h^3 cos t sum_j w_j eta_x(s_j) - h cos t (h tan e1 eta_b(entrance) + h tan e2 eta_b(exit)), I4y with sin t and eta_y;
 *       h tan e are the edge constants of the tracking (zero where the face's fringe is off): a rectangular magnet's path length
 *       does not grow with x
 *     I5u = L |h|^3 sum_j w_j H_u(s_j)
 *   The quadrature error for a bend of angle theta is of order theta^16 / 16!: about 1e-10 at theta = pi / 2 per Dipole.
 *   workspace: chx_dkd_ring_radiation_workspace_bytes(E) bytes, 16-byte aligned (chx_dkd_ring_jacobian's); 0 for E out of range.
 * Eight lanes per seed as in chx_dkd_ring_jacobian, one pass; at a Dipole the group evaluates the eight partial maps from the
 * entrance state (the one dual-number bend map on rebuilt constants), the sums over a seed's lanes stay in its wave, every
 * accumulation is float64 in a fixed order, no atomics. Two launches, none synchronising; two calls give the same bits and a
 * seed's rows do not depend on B. A seed whose orbit is NaN or whose image is not finite is NaN in all its rows.
 * CHX_ERR_INVALID_ARG, before any launch: the ring's conditions of chx_dkd_ring_jacobian, B < 1, a required pointer that is
 * NULL, integrals, along or the workspace sharing bytes with one another or with an input, a workspace too small or not 16-byte
 * aligned; CHX_ERR_DTYPE: dtype other than CHX_F32 / CHX_F64. (An additive export: CHX_ABI_VERSION stays as it is.) */
size_t chx_dkd_ring_radiation_workspace_bytes(int64_t E);
int chx_dkd_ring_radiation(const int32_t* kinds, const void* const* params, const int32_t* num_steps, const int32_t* fringe_at,
                           int64_t E, const void* energy_in, double mass_eV, double n_charges, int dtype, const double* orbit,
                           const double* beta0, const double* alpha0, const double* eta0, int64_t B, double* integrals,
                           double* along, void* workspace, size_t workspace_bytes, void* stream);
/* Backward of chx_dkd_track (the reference gets it from torch autograd through utils/bmadx.py): forward-mode dual
 * numbers on device, one seeded evaluation per input. dx[B][N][7] (dtype, may be NULL) = dY . d x_out / d x_in;
 * partials (may be NULL) = chx_dkd_bwd_partials_count() doubles laid out [B][ceil(N/256)][P + 1]: per workgroup
 * sums of dY . d x_out / d theta_k (k < P: params, k = P: energy) — the caller sums axis 1 (deterministic; no
 * atomics). The gradient of energy_out with respect to energy is the identity. */
int64_t chx_dkd_bwd_partials_count(int kind, int64_t B, int64_t N);
int chx_dkd_track_bwd(int kind, const void* x_in, const void* params, const void* energy, const void* dY,
                      double mass_eV, double n_charges, int32_t num_steps, int32_t fringe_at, int64_t B, int64_t Bx,
                      int64_t Bp, int64_t Be, int64_t N, int dtype, void* dx, double* partials, void* stream);

/* The reference's singularity-free special functions (utils/autograd.py:4-74, the torch.autograd.Function pairs at
 * :77-700) element-wise over n values, with their partial derivatives: out[i] = f(a[i] (, b[i])), da[i] = df/da,
 * db[i] = df/db (da / db may be NULL; b is ignored by the one-argument kinds). Evaluated in double, stored as dtype.
 *   LOG1PDIV log(1+x)/x            SI1MDIV (1 - si sqrt x)/x           SICOS1MDIV (1 - si sqrt x cos sqrt x)/x
 *   SIPSICOS3MDIV (3 - 4 si + si cos)/(2x)                             SICOSKUDDELMUDDEL15MDIV (utils/autograd.py:305-308)
 *   COSSQRTMCOSDIVDIFF (cos sqrt b - cos sqrt a)/(a - b)               SIMSIDIVDIFF (si sqrt a - si sqrt b)/(b - a)
 *   SI2MSI2DIVDIFF (si^2 sqrt b - si^2 sqrt a)/(a - b)                 SQRTA2MINUSBDIVA (sqrt(a^2 + b) - a)/b
 * with si x = sin x / x, negative arguments continued through the hyperbolic forms, and the limits at x = 0, a = b,
 * b = 0 the reference substitutes. */
enum chx_special_kind {
    CHX_SP_LOG1PDIV = 0, CHX_SP_SI1MDIV = 1, CHX_SP_SICOS1MDIV = 2, CHX_SP_SIPSICOS3MDIV = 3,
    CHX_SP_SICOSKUDDELMUDDEL15MDIV = 4, CHX_SP_COSSQRTMCOSDIVDIFF = 5, CHX_SP_SIMSIDIVDIFF = 6,
    CHX_SP_SI2MSI2DIVDIFF = 7, CHX_SP_SQRTA2MINUSBDIVA = 8
};
int chx_special(int kind, const void* a, const void* b, int64_t n, int dtype, void* out, void* da, void* db,
                void* stream);

/* Second-order tracking (element.py:195-228): x_out_i = sum_jk T_ijk x_j x_k with the MAD-convention
 * tensors of track_methods.py:80-296 (base_ttensor), the first-order map filled into T[:, 6, :] and the
 * element's rotations / misalignments / fringes folded in (drift.py:68-84, quadrupole.py:113-146,
 * dipole.py:397-428, sextupole.py:91-116). params[Bp][P] (dtype):
 *   CHX_T_DRIFT [length]   CHX_T_QUADRUPOLE [length, k1, tilt, mx, my]   CHX_T_SEXTUPOLE [length, k2, tilt, mx, my]
 *   CHX_T_DIPOLE = the CHX_DIPOLE vector [length, angle, k1, e1, e2, tilt, fint, fint_exit, gap]
 *   CHX_T_GENERAL [length, k1, k2, hx]: the bare tensor of track_methods.base_ttensor (track_methods.py:80-281) for any
 *   combination of the three strengths, without a first-order block and without dressing (custom elements)
 * T_out[B][7][7][7] (dtype). */
enum chx_t_kind { CHX_T_DRIFT = 0, CHX_T_QUADRUPOLE = 1, CHX_T_DIPOLE = 2, CHX_T_SEXTUPOLE = 3, CHX_T_GENERAL = 4 };
int chx_t_num_params(int kind);
int chx_build_ttensor(int kind, const void* params, const void* energy, double mass_eV, int64_t B, int64_t Bp,
                      int64_t Be, int dtype, void* T_out, void* stream);
int chx_apply_second_order(const void* x_in, const void* T, void* x_out, int64_t B, int64_t Bx, int64_t BT,
                           int64_t N, int dtype, void* stream);
/* A run of E elements tracked with their second-order maps on one beam x_in[N][7] (a lattice with tracking_method =
 * "second_order": element.py:195-228 once per element): HOST arrays T_maps[E] (device pointers to each element's [7][7][7] map)
 * and lengths[E] (device pointers to the elements' length scalars, only read when s_in / s_out are given: s_out = (((s_in +
 * l_0) + l_1) + ...) in dtype). x_tmp[N][7] is scratch (may be NULL for E = 1). Two launches per 224 elements, the particles in
 * registers across the run (x_tmp holds the folded coefficients, 256 per element); a beam too small for that scratch: E
 * launches. Either way one call and the values of E separate chx_apply_second_order calls (an exact zero may differ in sign). */
int chx_second_order_chain(const void* const* T_maps, const void* const* lengths, int64_t E, const void* x_in, int64_t N, int dtype,
                           void* x_out, void* x_tmp, const void* s_in, void* s_out, void* stream);
/* The same run with first-order maps in between: linear[E] (HOST array, may be NULL) marks T_maps[e] as a [7][7] map — a merged
 * run of linear elements between second-order ones (segment.py:545-574 tracks it with its composed map) — applied with the
 * arithmetic of chx_apply_affine7; lengths[e] is then the run's summed length. One pass over the beam for the whole stretch. */
int chx_second_order_chain_mixed(const void* const* T_maps, const int32_t* linear, const void* const* lengths, int64_t E,
                                 const void* x_in, int64_t N, int dtype, void* x_out, void* x_tmp, const void* s_in, void* s_out,
                                 void* stream);
/* The same run as a RING: turns [first_turn, first_turn + num_turns) (1-based) of the E items in one particle launch, the particles
 * in registers from turn to turn. T_maps / linear / lengths as above, 1 <= E <= 224.
 *   lost_turn[N] (int32, in / out): 0 = alive, else the turn the particle was lost on. At the end of every turn a live particle is
 *     lost when one of its six coordinates is non-finite or, with aperture[2] (device, dtype; NULL: none) given, |x| > aperture[0]
 *     or |y| > aperture[1]. It keeps the coordinates of that moment and is not tracked further.
 *   Every turn t with t % record_every == 0 is record t / record_every - 1: sums[record][14] (float64) = count, sum w, sum w x_j,
 *     sum w x_j^2 (j < 6) over the live particles, w = (double)charges[n] * (double)survival[n] (either may be NULL: 1), added
 *     in a fixed order (bitwise reproducible); probe[record][K][7] (dtype) = the first K rows of the beam, 0 <= K <= N. The call
 *     writes the rows of the records that fall into its turns; sums / probe point at record 0.
 *   x_out must not be x_in when first_turn == 1; a later chunk runs in place (x_in == x_out). No other two buffers may alias.
 *   s_in / s_out (dtype scalars, both or neither): s_out = (((s_in + l_0) + l_1) + ...), the path length after ONE turn.
 *   workspace: chx_second_order_turns_workspace_bytes(E, N, records of this call, dtype) bytes (the folded coefficients and the
 *     per-workgroup partial sums), 16-byte aligned.
 * CHX_ERR_INVALID_ARG: E < 1, E > 224, num_turns < 1, record_every < 1, K > N, a last turn of 2^31 - 1 or beyond, aliased buffers, a
 * workspace too small or not 16-byte aligned; CHX_ERR_DTYPE: dtype other than CHX_F32 / CHX_F64. */
size_t chx_second_order_turns_workspace_bytes(int64_t E, int64_t N, int64_t records_in_chunk, int dtype);
int chx_second_order_turns(const void* const* T_maps, const int32_t* linear, const void* const* lengths, int64_t E, const void* x_in,
                           const void* charges, const void* survival, int64_t N, int dtype, int64_t first_turn, int64_t num_turns,
                           int64_t record_every, const void* aperture, int64_t K, void* x_out, int32_t* lost_turn, double* sums,
                           void* probe, const void* s_in, void* s_out, void* workspace, size_t workspace_bytes, void* stream);
/* Derivatives of the two calls above (reference: torch autograd through track_methods.py:80-296 and the einsum).
 * chx_build_ttensor_vjp: dparams[B][P], denergy[B] (dtype) = dT[B][343] . dT/dtheta (dual numbers, one workgroup
 * per (row, input)); rows are NOT reduced when params / energy are broadcast (Bp or Be = 1) — the caller sums.
 * chx_apply_second_order_bwd: dx[B][N][7] (dtype, may be NULL) and dU_partials (may be NULL) =
 * chx_second_order_bwd_partials_count(B) doubles [B][256][196]: partial sums of dY_i x_j x_k over particles for
 * j <= k in the order (i, (0,0),(0,1)..(0,6),(1,1)..(6,6)); dT_ijk = dT_ikj = sum over axis 1. */
int chx_build_ttensor_vjp(int kind, const void* params, const void* energy, double mass_eV, const void* dT, int64_t B,
                          int64_t Bp, int64_t Be, int dtype, void* dparams, void* denergy, void* stream);
int64_t chx_second_order_bwd_partials_count(int64_t B);
int chx_apply_second_order_bwd(const void* x_in, const void* T, const void* dY, void* dx, double* dU_partials,
                               int64_t B, int64_t Bx, int64_t BT, int64_t N, int dtype, void* stream);

/* ---- Aperture (aperture.py:90-135): survival_out[B][N] = survival_in * inside, with
 * limits[Bl][2] = (x_max, y_max); rectangular uses strict inequalities, elliptical x^2/x_max^2 + y^2/y_max^2 <= 1,
 * both evaluated in `dtype`. survival_in may be NULL (all ones). */
enum chx_aperture_shape { CHX_APERTURE_RECTANGULAR = 0, CHX_APERTURE_ELLIPTICAL = 1 };
int chx_aperture_mask(const void* x_in, const void* survival_in, const void* limits, int shape, int64_t B, int64_t Bx,
                      int64_t Bs, int64_t Bl, int64_t N, int dtype, void* survival_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CHX_H */
