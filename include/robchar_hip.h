/* robchar_hip.h - C ABI of librobchar_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the Monte-Carlo robustness-characterisation hot path of RobChar.  The
 * reference is pure Python and has no FFI layer; each entry point below replaces a Python loop nest of the
 * reference and is what a ctypes binding on the reference side would call:
 *
 *   rc_mc_fidelity_f64*   replaces LOOP 2 x LOOP 3 of MCDataSim.get_algo_fid_dist (mcsim.py:434-456), i.e.
 *                         C x K calls of noise_model_base.evaluate_noisy_fidelity(x, ham_noisy=True)
 *                         (noise_model.py:98-109) with structured_perturbation.perturbation
 *                         (noise_model.py:122-147), for ONE sigma_sim level.
 *   rc_reduce_f64*        replaces the per-controller metric maps of mcsim.py:144-183 as applied in
 *                         get_metric_dict_from_scratch (mcsim.py:480-500): RIM_1 = wd_from_ideal
 *                         (wd_sortof_fast_implementation.py:82-116), np.std, min, Q(threshold), each for
 *                         the centre / DKW-upper / DKW-lower tensors, plus the sorted sample (ECDF).
 *                         rim1 (= 1 - mean_k fidelity) is also the reduction of NStochOpt.get_rims
 *                         (gen_fig_8_arim_fcall_scaling.py:121-132).
 *   rc_rim_p_f64*         replaces RIM_p (wd_sortof_fast_implementation.py:147-174).
 *   rc_mc_*_sharded_f64   the same loops over all GPUs of a node from one process (the role of the reference's dead
 *                         multiprocessing.Pool, mcsim.py:451-455): controller blocks, host arrays in / out.
 *   rc_draws_legacy_f64   the reference's RNG itself - NumPy's legacy RandomState normal stream (noise_model.py:114-115,
 *                         :137-146, the burned draw of mcsim.py:425) - continued on the device, state handed back.
 *   rc_directional_draws_legacy   the interleaved randint / normal(size=2) consumption of directional_perturbation
 *                         (noise_model.py:183-189) on the same stream, on the host; rc_directional_draws_legacy_dev: the
 *                         same with the word stream, the per-position parse and the normals on the device.
 *   rc_draws_philox_f64*  counter-based draws for sample spaces too large for a sequential stream (not the reference's RNG).
 *   rc_json_*             json.dump of the fidelity / metric tensors into the .mc / .mcm caches (mcsim.py:457-459, :501).
 *
 * Conventions: every function returns 0 on success and a negative RC_E* code on failure, with a
 * human-readable message available from rc_last_error() (thread-local).  The caller owns every buffer.
 * All inputs, outputs and results are IEEE fp64, accurate to the 1e-10 the reference's complex128 path is matched to (in
 * practice ~1e-15).  Internally the chain kernels compute their eigenvalue STARTING VALUES in fp32 (N = 3..13) and finish
 * them in fp64; nothing of fp32 accuracy reaches a result.  No Python / torch types cross this boundary.
 *
 * Data layout (row-major, fp64):
 *   controllers [C][N+1]      x[0..N-1] = biases, x[N] = time (abs() is taken, noise_model.py:99).
 *                             A row containing NaN marks a padded controller (mcsim.py:442-443):
 *                             its K outputs are NaN and its draws are not read.
 *   draws       [C][K][N][3]  (g0_i, g1_i, g2_i) per site i in the order the reference consumes its RNG
 *                             (noise_model.py:137-146), ALREADY scaled by sigma_sim.  g1_0, g2_0 are ignored.
 *   fid_out     [C][K]
 *   h0_diag     [N] or NULL   static diagonal added to every sample (NULL = 0; the XXZ term of
 *                             qnewton.py:148-150 goes here).  HOST pointer.
 *   h0_offdiag  [N-1] or NULL static couplings (NULL = 1.0, noise_model.py:80-82).  HOST pointer.
 *
 * Alignment of device pointers: that of the element type (8 bytes for fp64 and 64-bit integers, 4 for int32) and nothing
 * more - an array may start at any element of a larger allocation.  Where an array sits changes no result (same inputs,
 * same bits), and no entry reads or writes outside the arrays it is given (tests/test_gpu_placement.py).
 */
#ifndef ROBCHAR_HIP_H
#define ROBCHAR_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define RC_ABI_VERSION 20     /* 2: + multi-device entries, legacy-stream draws, JSON cache encoder, RC_KERNEL_RING_HH;
                                  3: + rc_stats_polish_tiles; 4: + rc_directional_draws_legacy_dev;
                                  5: + rc_reserve_ring, rc_release_stream, rc_mc_fidelity_directional_f64_async,
                                     rc_mc_fidelity_philox_f64_async;
                                  6: + rc_build_flags, rc_philox_fused_pays, rc_reduce_ex_f64_async,
                                     rc_legacy_log_is_host_exact, rc_comm_init / rc_comm_size / rc_comm_destroy /
                                     rc_mc_metrics_gathered_f64 (all additive);
                                  7: + rc_mc_fidelity_grad_f64_async, rc_mc_fidelity_grad_f64, rc_stats_grad_general_tiles,
                                     RC_MAX_NSPIN_GRAD (additive);
                                  8: + rc_mc_fidelity_sens_f64_async, rc_mc_fidelity_sens_f64, rc_stats_sens_general_tiles
                                     (additive);
                                  9: + rc_mc_fidelity_sens_philox_f64_async (additive);
                                  10: + rc_mc_fidelity_grad_philox_f64_async (additive);
                                  11: + rc_mc_fidelity_grad_listed_f64_async (additive);
                                  12: + rc_tail_select_len, rc_tail_select_f64_async (additive);
                                  13: + rc_lbfgs_state_len, rc_lbfgs_init_f64_async, rc_lbfgs_advance_f64_async,
                                      rc_lbfgs_result_f64_async (additive);
                                  14: + rc_lbfgs_init_box_f64_async, rc_lbfgs_advance_box_f64_async (additive);
                                  15: + rc_bootstrap_metrics_f64_async, rc_bootstrap_metrics_f64 (additive);
                                  16: + rc_mc_fidelity_times_f64_async, rc_mc_fidelity_times_f64,
                                      rc_mc_fidelity_times_philox_f64_async, rc_stats_times_general_tiles, RC_MAX_TIMES (additive);
                                  17: + rc_mc_fidelity_grad_times_philox_f64_async (additive);
                                  18: + rc_wasserstein_matrix_f64_async, rc_wasserstein_matrix_f64 (additive);
                                  19: + rc_sobol_dirnum_u32, rc_draws_sobol_f64_async, rc_draws_sobol_f64,
                                      rc_mc_fidelity_sobol_f64_async, RC_SOBOL_MAX_DIM, RC_MAX_NSPIN_SOBOL (additive);
                                  20: + rc_mc_fidelity_pickfreeze_philox_f64_async, RC_MAX_NSPIN_PICKFREEZE,
                                      RC_PICKFREEZE_MAX_GROUPS (additive) */
#define RC_MAX_NSPIN 32        /* chain topology: register-resident fast kernels for N <= RC_MAX_NSPIN_CHAIN, a general
                                 * LDS-resident per-sample kernel (same arithmetic, ~10x slower per site) above */
#define RC_MAX_NSPIN_FAST 16   /* limit of the dense kernels (RC_KERNEL_JACOBI, RC_KERNEL_EXPM: ring, non-Hermitian), of the
                                 * mixed-precision / fused-Philox chain kernels and of the rows-mode chain kernel */
#define RC_MAX_NSPIN_CHAIN 24  /* (round 5) chains of 17 .. 24 spins: the register-resident eigenvalue-only kernel (all-fp64 QL +
                                 * adjugate weights, one wave per SIMD) instead of the LDS kernel: N = 17 at 1.2x the N = 16
                                 * time where the LDS kernel took 6x */

#define RC_MAX_NSPIN_GRAD 12   /* (ABI 7) limit of the fidelity-gradient kernel (chain topology).  Its QL carries eigenvector rows in
                                 * registers: all N up to N = 9, batches of 6 / 5 / 4 rows in 2 / 3 / 5 passes at N = 10 / 11 / 12; the
                                 * pass count, not a register limit, is what ends the list here */

#define RC_SOBOL_MAX_DIM 96    /* (ABI 19) dimensions of the Sobol table: the 3 N coordinates of chains of up to 32 spins */
#define RC_MAX_NSPIN_SOBOL 13  /* (ABI 19) limit of the fidelity kernel that generates its Sobol normals itself (chain topology) */
#define RC_MAX_NSPIN_PICKFREEZE 13   /* (ABI 20) limit of the pick-freeze kernel of the variance indices (chain topology) */
#define RC_PICKFREEZE_MAX_GROUPS 64  /* (ABI 20) groups of noise coordinates per call of that kernel */

#define RC_OK 0
#define RC_EINVAL (-1)   /* bad argument (N out of range, in/out out of range, NULL pointer, ...) */
#define RC_EHIP (-2)     /* a HIP runtime call failed; rc_last_error() carries hipGetErrorString */
#define RC_ENOSUP (-3)   /* valid request that this build does not implement */

/* kernels selectable through rc_set_fidelity_kernel / the `kernel` argument */
#define RC_KERNEL_AUTO 0      /* chain -> TRIDIAG_ADJ; ring -> the mixed-precision lane-per-sample route + RING_HH as its repair (N <= 16) */
#define RC_KERNEL_TRIDIAG_QL 1 /* lane-per-sample real-symmetric-tridiagonal implicit QL (chain only) */
#define RC_KERNEL_TRIDIAG_ADJ 3 /* same QL on eigenvalues only; eigenvector weights from the adjugate of (lambda I - H) (chain only) */
#define RC_KERNEL_EXPM 4       /* dense complex Pade scaling-and-squaring expm in LDS, one wavefront per sample (any topology) */
#define RC_KERNEL_JACOBI 2     /* complex Hermitian cyclic Jacobi in LDS, one wavefront per sample (chain or ring) */
#define RC_KERNEL_RING_HH 5    /* ring only: lane-per-sample reduction to tridiagonal form in registers (N <= 10: dense Householder;
                                 * N = 11 .. 16, round 5: the ring folded into a pentadiagonal band + band reduction) + the QL of the chain kernels */

int rc_version(void);
int rc_device_count(void);
const char* rc_last_error(void);

/* (ABI 6) Compile-time switches of THIS build that change results or remove a safety net; 0 = the product build.  The
 * four RC_BUILD_EXPERIMENT_* bits are RESERVED: no switch of this tree sets them; only timing-experiment builds of earlier trees
 * do, and those knowingly return wrong fidelities for some samples - a loader must go on refusing them (code-robchar_amd/_lib.py
 * does, unless ROBCHAR_ALLOW_EXPERIMENT_LIB=1). */
#define RC_BUILD_EXPERIMENT_NO_STEPPING 1
#define RC_BUILD_EXPERIMENT_STEP_NOT_RUN 2
#define RC_BUILD_EXPERIMENT_FALLBACK_NOT_RUN 4
#define RC_BUILD_EXPERIMENT_PHILOX_NOSTORE 8
#define RC_BUILD_DEV_FEW_N 16            /* chain kernels for N = 5, 7, 10 only (kernel-tuning builds) */
#define RC_BUILD_STAMPS 32               /* per-wave s_memtime stamps compiled in */
#define RC_BUILD_NO_SUM_RULE_GUARD 64    /* -DRC_SUM_RULE_GUARD=0 */
#define RC_BUILD_NO_KEEP_SETTLED 128     /* -DRC_KEEP_SETTLED=0 */
#define RC_BUILD_WRONG_RESULTS_MASK 15   /* the bits under which some results are knowingly wrong */
int rc_build_flags(void);

/* Blocking call.  `controllers`, `draws`, `fid_out` may each be a host pointer or a device pointer on
 * `device` (detected with hipPointerGetAttributes); host buffers are staged through an internal per-device
 * workspace.  Runs on an internal per-device stream and returns after the result is in `fid_out`. */
int rc_mc_fidelity_f64(int device, int N, int in, int out,
                       const double* h0_diag, const double* h0_offdiag, int ring,
                       const double* controllers, const double* draws,
                       long long C, long long K, double* fid_out);

/* Same, with an explicit kernel choice (RC_KERNEL_*) instead of the process-wide default. */
int rc_mc_fidelity_kernel_f64(int device, int kernel, int N, int in, int out,
                              const double* h0_diag, const double* h0_offdiag, int ring,
                              const double* controllers, const double* draws,
                              long long C, long long K, double* fid_out);

/* Enqueue-only variant: all three arrays are DEVICE pointers on `device`; the kernel is launched on
 * `stream` (a hipStream_t; NULL = the device's default stream) and the call returns without synchronising.
 * `kernel` is one of RC_KERNEL_*. */
int rc_mc_fidelity_f64_async(int device, void* stream, int kernel, int N, int in, int out,
                             const double* h0_diag, const double* h0_offdiag, int ring,
                             const double* controllers_dev, const double* draws_dev,
                             long long C, long long K, double* fid_out_dev);

/* Ring topology through the enqueue-only entries (ring = 1, N <= 16, RC_KERNEL_AUTO): the mixed-precision route lists the
 * samples it does not trust itself with and a repair launch behind it recomputes them; list and counters live in a buffer
 * the library keeps per (device, stream), allocated, zeroed, grown and released IN STREAM ORDER on that stream - an enqueue
 * never synchronises the device.  (ABI 5)
 *   rc_reserve_ring(device, stream, samples): size that buffer for launches of up to `samples` = C * K now, e.g. outside a
 *     latency-critical region (otherwise the first ring launch on the stream, or a larger one, enqueues the allocation).
 *   rc_release_stream(device, stream): hand the stream's buffer back (stream-ordered free behind its last launch); call
 *     before destroying a stream that ran ring launches.  Both return RC_OK when there is nothing to do. */
int rc_reserve_ring(int device, void* stream, long long samples);
int rc_release_stream(int device, void* stream);

/* Extended enqueue-only variant: `draws_ctrl_stride` is the distance, in doubles, between the draw blocks of
 * consecutive controllers: K*N*3 (or any larger pitch) = every controller has its own K draws, as above;
 * 0 = ONE set of K draws [K][N][3] shared by every controller.  The shared form is the optimiser-side noisy
 * objective of the reference (qnewton.py:383-444, `fidelity_ss_av` over the fixed Hamiltonian sets built by
 * `randHset_constructor`, qnewton.py:122-137), whose perturbation is real (2 draws per site: set g2 = 0). */
int rc_mc_fidelity_ex_f64_async(int device, void* stream, int kernel, int N, int in, int out,
                                const double* h0_diag, const double* h0_offdiag, int ring,
                                const double* controllers_dev, const double* draws_dev,
                                long long draws_ctrl_stride, long long C, long long K, double* fid_out_dev);

/* (ABI 7) Fidelity AND its gradient with respect to the controller x = [B_0 .. B_{N-1}, T], chain topology,
 * N = 2 .. RC_MAX_NSPIN_GRAD (RC_ENOSUP above, with a message; rings are not covered):
 *     F = |<out| exp(-i |x_N| H) |in>|^2,   H = HH + Z(draws) + diag(x_0 .. x_{N-1}),
 *     dF/dx_l (l < N) and dF/dx_N = sign(x_N) dF/dT (0 at x_N = 0)
 * - what the reference's L-BFGS consumes (qnewton.py:162-212) - per sample, and their means over the K samples of a controller
 * row (the optimiser-side objective `fidelity_ss_av` and its gradient when draws_ctrl_stride = 0: one draw set shared by all
 * controllers).  One kernel launch (plus a small second pass for the means) instead of the 2 (N + 1) launches of central
 * differences; accurate to the fidelity's own bar times one factor of T (biases) or ||H|| (time entry).
 * Outputs, each optional (NULL = not wanted; all three NULL: RC_EINVAL "no output"):
 *     fid_out  [C][K]        the fidelities.  Computed from the same eigensystem as the gradient (all-fp64 QL with eigenvector
 *                            rows), NOT by the RC_KERNEL_AUTO route: the two agree to rounding (<= 1e-12 observed; both are held
 *                            to 1e-10 against the oracle), not bit for bit;
 *     grad_out [C][K][N+1]   the per-sample gradients;
 *     mean_out [C][N+2]      (mean F, mean dF/dx_0 .. mean dF/dx_N) over the K samples of the row.  Deterministic: fixed
 *                            summation order, no atomics - the same inputs give the same bits on every run.
 * A controller row that contains a NaN gives NaN in all three outputs and reads no draws.  `draws_ctrl_stride` as in
 * rc_mc_fidelity_ex_f64_async (negative = K*N*3).  Arguments are validated before any HIP call; C = 0 or K = 0: RC_OK, nothing
 * written.  Enqueue-only: device pointers, launched on `stream`; the per-tile partial sums of the means live in a
 * stream-ordered allocation (hipMallocAsync / hipFreeAsync on `stream`), so the call never synchronises the device.
 * Stream capture (hipGraph, torch.cuda.graph): with mean_out = NULL the call enqueues one kernel and nothing else and may be
 * captured; with mean_out set it allocates during the call - capturing that is untested and not supported. */
int rc_mc_fidelity_grad_f64_async(int device, void* stream, int N, int in, int out,
                                  const double* h0_diag, const double* h0_offdiag,
                                  const double* controllers_dev, const double* draws_dev, long long draws_ctrl_stride,
                                  long long C, long long K, double* fid_out_dev, double* grad_out_dev, double* mean_out_dev);

/* Blocking form of the above: every array may be a host pointer or a device pointer on `device`, as in rc_mc_fidelity_f64.
 * `draws` holds C*K*N*3 doubles, or K*N*3 when draws_ctrl_stride = 0. */
int rc_mc_fidelity_grad_f64(int device, int N, int in, int out,
                            const double* h0_diag, const double* h0_offdiag,
                            const double* controllers, const double* draws, long long draws_ctrl_stride,
                            long long C, long long K, double* fid_out, double* grad_out, double* mean_out);

/* Diagnostic (ABI 7): tiles of the gradient kernel in which some sample's QL hit the sweep cap and took the textbook
 * per-sample routine since the last reset (never observed). */
long long rc_stats_grad_general_tiles(int device, int reset);

/* (ABI 8) Fidelity AND its derivatives with respect to the structured noise, i.e. the sample's OWN DRAWS, chain topology,
 * N = 2 .. RC_MAX_NSPIN_GRAD (RC_ENOSUP above; rings are not covered).  With H = HH + Z(g) + diag(x), Z[i][i] = g0_i,
 * Z[i][i-1] = g1_i + i g2_i (i >= 1), the 3 N - 2 directions are the N site energies, the N - 1 real and the N - 1 imaginary
 * couplings - the list `directional_perturbation` draws from.  From the eigensystem of the gradient kernel:
 *     dF/dg0_i = dF/dx_i,    dF/dg1_i = (re_i / r_i) dF/dr_i,    dF/dg2_i = (im_i / r_i) dF/dr_i,
 * re_i + i im_i the complex coupling of the sites i-1, i and r_i its modulus; both coupling derivatives are exactly 0 at an
 * exactly cut bond (r_i = 0), which is their true value.  Per sample the radial derivative is rho = sum_{i,c} g_{i,c} dF/dg_{i,c};
 * for draws g = sigma z its row mean is dFbar/dln(sigma) at that sigma (sigma itself never enters).
 * Outputs, each optional (NULL = not wanted; all three NULL: RC_EINVAL "no output"):
 *     fid_out  [C][K]         the fidelities (from the kernel's own eigensystem, as in rc_mc_fidelity_grad_f64_async);
 *     sens_out [C][K][N][3]   dF/dg in the draws' own layout; the entries [0][1] and [0][2] are 0;
 *     mean_out [C][3N+2]      (mean F, mean rho, then the N x 3 mean dF/dg) over the K samples of the row.  Deterministic: fixed
 *                             summation order, no atomics.
 * NaN rows, `draws_ctrl_stride` (0 = one draw set shared by all controllers), argument checks before any HIP call, empty
 * batches, the stream-ordered scratch allocation behind mean_out and stream capture: as in rc_mc_fidelity_grad_f64_async. */
int rc_mc_fidelity_sens_f64_async(int device, void* stream, int N, int in, int out,
                                  const double* h0_diag, const double* h0_offdiag,
                                  const double* controllers_dev, const double* draws_dev, long long draws_ctrl_stride,
                                  long long C, long long K, double* fid_out_dev, double* sens_out_dev, double* mean_out_dev);

/* Blocking form of the above: every array may be a host pointer or a device pointer on `device`. */
int rc_mc_fidelity_sens_f64(int device, int N, int in, int out,
                            const double* h0_diag, const double* h0_offdiag,
                            const double* controllers, const double* draws, long long draws_ctrl_stride,
                            long long C, long long K, double* fid_out, double* sens_out, double* mean_out);

/* Diagnostic (ABI 8): the counter of rc_stats_grad_general_tiles for the noise-sensitivity kernel. */
long long rc_stats_sens_general_tiles(int device, int reset);

/* The same fidelities with the COUNTER-BASED draws generated inside the kernel (ABI 5; SURVEY.md 8(d): "in philox mode draws
 * are not read"): sample (c, k), site i, slot s is element  offset + ((c K + k) N + i) 3 + s  of stream `seed` - exactly what
 * rc_draws_philox_f64_async(seed, offset, C K N 3, sigma) would have written, by the same routine, so the result is BIT-IDENTICAL
 * to generating the [C][K][N][3] tensor and calling rc_mc_fidelity_f64_async on it; only that tensor (24 N bytes per sample:
 * 16.8 GB for BASELINE config 4) never exists.  `sigma_rows_dev` [C] (or NULL: `sigma` for every row): scale per controller row,
 * so that all sigma levels of an algorithm go through one launch with the controller rows tiled.  Chain topology, the
 * eigenvalue-only kernels (kernel = RC_KERNEL_AUTO or RC_KERNEL_TRIDIAG_ADJ), N <= RC_MAX_NSPIN_FAST; RC_ENOSUP otherwise
 * (generate the tensor instead).  It is the faster route up to N = 13 (0.70 - 0.86 of the two-kernel route's time) and for
 * end-to-end pairs at N = 14; beyond that the two-kernel route is ~7 % faster.  Enqueue-only.  This replaces LOOP 2 x LOOP 3 of mcsim.py:434-456 together with the
 * perturbation draws of noise_model.py:122-147 for callers who do not need the reference's RNG stream. */
int rc_mc_fidelity_philox_f64_async(int device, void* stream, int kernel, int N, int in, int out,
                                    const double* h0_diag, const double* h0_offdiag, const double* controllers_dev,
                                    unsigned long long seed, unsigned long long offset, double sigma,
                                    const double* sigma_rows_dev, long long C, long long K, double* fid_out_dev);

/* (ABI 9) The noise sensitivity of rc_mc_fidelity_sens_f64_async with the COUNTER-BASED draws generated inside the kernel, as
 * rc_mc_fidelity_philox_f64_async does for the fidelities.  Stream convention: sample (c, k), site i, slot s is element
 *     offset + ((c K + k) N + i) 3 + s   of stream `seed`,
 * scaled by `sigma`, or by sigma_rows_dev[c] when that is not NULL (one scale per controller row: all sigma levels of an
 * algorithm go through ONE launch with the controller rows tiled) - exactly what rc_draws_philox_f64_async(seed, offset, C K N 3,
 * sigma) would have written, by the same routine.  fid_out, sens_out and mean_out are BIT-IDENTICAL to generating that
 * [C][K][N][3] tensor and calling rc_mc_fidelity_sens_f64_async on it (same per-sample arithmetic, same summation order of the
 * row means); only the tensor - 24 N bytes per sample - never exists.
 * The radial derivative rho = sum g dF/dg is taken over the GENERATED draws g = sigma z, so its row mean in mean_out[c][1] is
 * dFbar/dln(sigma) at that row's sigma.  A row with sigma = 0 yields the nominal sensitivity (dF/dg of the unperturbed system in
 * every one of its K samples) with rho = 0 exactly.
 * Outputs (each optional; all three NULL: RC_EINVAL), NaN rows (NaN everywhere, no draws generated), empty batches (C = 0 or
 * K = 0: RC_OK, nothing written), argument checks before any HIP call, the stream-ordered scratch allocation behind mean_out and
 * stream capture: as in rc_mc_fidelity_sens_f64_async.  With sigma_rows_dev = NULL a negative or non-finite `sigma` is RC_EINVAL
 * (with sigma_rows_dev set, `sigma` is not read).  Chain topology, N = 2 .. RC_MAX_NSPIN_GRAD (RC_ENOSUP above: "N <= 12").
 * The sweep-cap fallback counts into rc_stats_sens_general_tiles.  Enqueue-only: device pointers, launched on `stream`. */
int rc_mc_fidelity_sens_philox_f64_async(int device, void* stream, int N, int in, int out,
                                         const double* h0_diag, const double* h0_offdiag, const double* controllers_dev,
                                         unsigned long long seed, unsigned long long offset, double sigma,
                                         const double* sigma_rows_dev, long long C, long long K,
                                         double* fid_out_dev, double* sens_out_dev, double* mean_out_dev);

/* (ABI 10) The fidelity gradient of rc_mc_fidelity_grad_f64_async with the COUNTER-BASED draws generated inside the kernel, and on
 * request the second-moment sums from which the gradient of the row's variance follows.  Two stream conventions, chosen by
 * `shared_draws`:
 *     shared_draws = 0 (per-controller draws): sample (c, k), site i, slot s is element
 *         offset + ((c K + k) N + i) 3 + s   of stream `seed`;
 *     shared_draws != 0 (shared draws, common random numbers - the fidelity_ss_av objective): the element is
 *         offset + (k N + i) 3 + s,   the same for every c.
 * In both the scale is `sigma`, or sigma_rows_dev[c] when that is not NULL (one scale per controller row) - by the routine of
 * rc_draws_philox_f64_async.  fid_out, grad_out and mean_out are BIT-IDENTICAL to the two-kernel route: generating the
 * [C][K][N][3] tensor (shared draws: the one [K][N][3] set, draws_ctrl_stride = 0) with rc_draws_philox_f64_async(seed, offset, .,
 * sigma) and calling rc_mc_fidelity_grad_f64_async on it (same per-sample arithmetic, same summation order of the row means);
 * only the tensor - 24 N bytes per sample - never exists.  A row with sigma = 0 gives K identical samples.
 * Outputs, each optional (NULL = not wanted; all four NULL: RC_EINVAL "no output"):
 *     fid_out    [C][K], grad_out [C][K][N+1], mean_out [C][N+2]: as in rc_mc_fidelity_grad_f64_async;
 *     moment_out [C][N+2]   (mean F^2, mean F dF/dx_0 .. mean F dF/dx_N) over the K samples of the row, every product rounded
 *                           once, same fixed summation order as mean_out, no atomics: same inputs, same bits.  With mean_out:
 *                           grad Var F = 2 (mean F dF/dx - mean F mean dF/dx), Var F = mean F^2 - (mean F)^2 (ddof = 0).  With
 *                           moment_out = NULL the kernel does none of that work.
 * NaN rows (NaN in every output, no draws generated), empty batches (C = 0 or K = 0: RC_OK, nothing written), argument checks
 * before any HIP call and the stream-ordered scratch allocation behind mean_out / moment_out: as in
 * rc_mc_fidelity_sens_philox_f64_async.  With sigma_rows_dev = NULL a negative or non-finite `sigma` is RC_EINVAL (with
 * sigma_rows_dev set, `sigma` is not read).  Chain topology, N = 2 .. RC_MAX_NSPIN_GRAD (RC_ENOSUP above: "N <= 12").  The
 * sweep-cap fallback counts into rc_stats_grad_general_tiles.  Enqueue-only: device pointers, launched on `stream`.
 * Timing against the two-kernel route: DESIGN.md ("Gradient kernel with its own draws"); no automatic routing anywhere. */
int rc_mc_fidelity_grad_philox_f64_async(int device, void* stream, int N, int in, int out,
                                         const double* h0_diag, const double* h0_offdiag, const double* controllers_dev,
                                         unsigned long long seed, unsigned long long offset, double sigma,
                                         const double* sigma_rows_dev, int shared_draws, long long C, long long K,
                                         double* fid_out_dev, double* grad_out_dev, double* mean_out_dev, double* moment_out_dev);

/* (ABI 11) rc_mc_fidelity_grad_philox_f64_async over a caller-chosen LIST of each row's K draws, with caller-chosen weights on
 * the row sums:   sum_out[c] = sum_s  w[c][s] * (F, dF/dx_0 .. dF/dx_N)(c, list[c][s]),   s = 0 .. L - 1.
 * Tail weights on the worst alpha K draws give CVaR_alpha and its gradient (noise.tail_weights; on the device, without
 * torch: rc_tail_select_f64_async below, which writes list_dev and weight_dev from the fidelities), softmax weights the entropic
 * risk, a smoothed step's derivative a yield; repeated indices (bootstrap resamples) are allowed.  Only the listed samples are
 * computed.  Slot s of row c is sample (c, k = list_dev[c][s]) of the stream conventions above (`shared_draws`, `offset`, `sigma` /
 * sigma_rows_dev[c]): offset + ((c K + k) N + i) 3 + s', shared draws offset + (k N + i) 3 + s'.  A value outside 0 .. K - 1 is an
 * EMPTY slot: NaN in fid_out / grad_out, nothing added to sum_out.
 * Outputs, each optional (all three NULL: RC_EINVAL "no output"):
 *     fid_out [C][L], grad_out [C][L][N+1]   per slot;
 *     sum_out [C][N+2]   the weighted sums above; weight_dev [C][L], or NULL: w = 1 (no multiplication).  Every product is rounded
 *                        once, the slots are added in a fixed order, no atomics: same inputs, same bits.  A row of only empty
 *                        slots gives 0.
 * A NaN controller row gives NaN in all three outputs.  A sample's fid and grad bits depend on (c, k) and the other arguments
 * only - not on L, not on the slot, not on what else is listed (every lane runs exactly the QL sweeps it would run alone).
 * Against rc_mc_fidelity_grad_philox_f64_async on all K draws a listed sample therefore AGREES TO ROUNDING, NOT BIT FOR BIT - not
 * even with list = 0 .. K - 1: there the whole wave votes the sweep count for each eigenvalue index, so a sample's last bits depend
 * on its 63 wave-mates, and a listed sample sits among other mates.  Tested bound on fid: 64 N eps max(1, T ||H||).
 * Argument checks before any HIP call, in the family's order and with its codes and texts; then L < 0: RC_EINVAL; C, K or L = 0:
 * RC_OK, nothing written; list_dev NULL: RC_EINVAL.  N = 2 .. RC_MAX_NSPIN_GRAD (RC_ENOSUP above: "N <= 12"), chain topology.
 * The sweep-cap fallback counts into rc_stats_grad_general_tiles.  sum_out's scratch is allocated and freed in stream order
 * (hipMallocAsync), as for mean_out above, and the same stream-capture rules hold.  Enqueue-only: device pointers, launched on
 * `stream`.  Timing: DESIGN.md ("Listed-sample gradient"); no automatic routing anywhere. */
int rc_mc_fidelity_grad_listed_f64_async(int device, void* stream, int N, int in, int out,
                                         const double* h0_diag, const double* h0_offdiag, const double* controllers_dev,
                                         unsigned long long seed, unsigned long long offset, double sigma,
                                         const double* sigma_rows_dev, int shared_draws, long long C, long long K,
                                         const int* list_dev, const double* weight_dev, long long L,
                                         double* fid_out_dev, double* grad_out_dev, double* sum_out_dev);

/* (ABI 12) The lower tail of every row of a fidelity table, selected on the device: the list and the weights that make
 * rc_mc_fidelity_grad_listed_f64_async's sum_out the CVaR_alpha of the row and its gradient, and the value at risk.  The definition
 * is noise.tail_weights (NumPy route); every output carries its bits.
 *     m = rc_tail_select_len(K, alpha) = min(K, ceil(alpha K))     host only, no HIP call; -1 on bad arguments (alpha not in (0, 1]
 *                                                                  or NaN, K negative or above 2^31 - 1).
 * The host computes, in double precision and in exactly this order,   ak = alpha * K,   m = min(K, (long long)ceil(ak)),
 * w_body = 1.0 / ak,   w_last = (ak - (m - 1)) / ak.   Outputs for row c of fid_dev [C][K]:
 *     list_out   [C][m] int32   the indices of the m smallest values of the row under the order (value, index): ties go to the
 *                               lower index, as in NumPy's stable sort.  They are written in ascending index order.
 *     weight_out [C][m]         optional (NULL = not wanted): w_body everywhere, and w_last on the slot that holds the m-th smallest
 *                               element in that order.  With ties at the threshold, that is the selected tied element with the
 *                               highest index.
 *     var_out    [C]            optional: the m-th smallest value itself.
 * -0.0 and +0.0 are equal (NumPy treats them so), and the index breaks the tie.  A row containing any NaN gives list = -1,
 * weight = 0.0, var = NaN.  No sort: a radix select over an order-preserving 64-bit key and a compaction in index order, one
 * workgroup per row (one wave for rows of up to 2048 values), no workspace, integer counts only - same inputs, same bits, and the
 * same on every route.
 * Argument checks before any HIP call: alpha not in (0, 1], or NaN: RC_EINVAL; C or K negative: RC_EINVAL; K > 2^31 - 1: RC_EINVAL;
 * C or K = 0: RC_OK, nothing written; fid_dev or list_out_dev NULL: RC_EINVAL.  Enqueue-only: device pointers, launched on `stream`,
 * no allocation, no synchronisation; may be captured.  The three-call CVaR sequence of a client without torch:
 * rc_mc_fidelity_philox_f64_async -> rc_tail_select_f64_async -> rc_mc_fidelity_grad_listed_f64_async. */
long long rc_tail_select_len(long long K, double alpha);
int rc_tail_select_f64_async(int device, void* stream, const double* fid_dev, long long C, long long K, double alpha,
                             int* list_out_dev, double* weight_out_dev, double* var_out_dev);

/* (ABI 13) Batched L-BFGS with a backtracking line search, one independent problem per controller row, as a state machine on
 * the device: the optimiser that consumes the C rows of value and gradient the gradient entries above write per launch.  The loop
 * of a client is   init;  repeat { gradient launch on trial_dev -> advance }  - enqueue-only on one stream, rows in different
 * phases (first value, accepted step, backtracking, done) in the same launch.  The definition is code-robchar_amd/lbfgs.py (NumPy):
 * every dot product accumulated sequentially over the variable index, every product rounded once, IEEE division and square root;
 * the kernels give its bits (a NaN's sign and payload excepted).
 *     ndim      variables per row, 3 .. 13: the controller row of N = 2 .. RC_MAX_NSPIN_GRAD spins (N biases, then T)
 *     m         pairs kept per row, 1 .. 8
 *     state_dev rc_lbfgs_state_len(C, ndim, m) = C (4 ndim + 2 m ndim + m + 11) doubles, caller-owned, laid out [field][C]; opaque
 *               to a client (lbfgs.field_offsets names the fields); rc_lbfgs_state_len is host only, -1 on bad arguments
 *     trial_dev [C][ndim]: the `controllers_dev` argument of the next gradient launch.  The row of a DONE row is all NaN, which the
 *               gradient entries skip (their NaN-row rule); a done row's state never changes again.
 * rc_lbfgs_init_f64_async: x0_dev [C][ndim] start rows; mask_dev [C][ndim] of 0.0 / 1.0 or NULL (= all free): the gradient is
 *     multiplied by it, so a masked variable never moves (fix T this way).  Bounds on the variables are not supported by this
 *     entry and rc_lbfgs_advance_f64_async: the boxed entries (ABI 14) below take them.  A start row with a NaN is done at once
 *     (status 5).
 * rc_lbfgs_advance_f64_async: one (value, gradient) per row, evaluated at trial_dev, from row_a_dev [C][ndim + 1]:
 *     kind 0  raw                  (f, g_0 .. g_{ndim-1}) as they are
 *     kind 1  one_minus            row_a = a `mean_out` row of the gradient entries or a `sum_out` row of the listed entry:
 *                                  f = 1 - a[0], g = -a[1 ..]
 *     kind 2  one_minus_plus_std   row_a = mean_out, row_b_dev [C][ndim + 1] = moment_out of rc_mc_fidelity_grad_philox_f64_async:
 *                                  f = (1 - mean F) + lam std F and its gradient, std by the arithmetic and the floor rule of
 *                                  noise.moments_from_sums.  row_b_dev and lam are read by kind 2 only.
 *     A trial point is accepted when its value is finite and f_trial <= f + (c1 t) g.d (Armijo); otherwise the step is halved; after
 *     more than `maxback` halvings the history is dropped once (steepest descent, first step min(1, 1 / |g|_2)), then the row ends.
 *     c1 in (0, 1); gtol on max |g_i|; ftol = 0 switches the value test off; maxiter >= 1 accepted steps.
 *     status: 0 running, 1 max |g_i| <= gtol, 2 fprev - f <= ftol max(|fprev|, |f|, 1), 3 maxiter reached, 4 line search failed,
 *     5 first value or gradient not finite, or a NaN start row.
 * rc_lbfgs_result_f64_async: the rows' results out of the state: x_out [C][ndim], f_out [C], g_out [C][ndim], status_out [C] int32,
 *     iters_out [C] and evals_out [C] int64 (accepted steps, evaluations consumed); each optional, RC_EINVAL "no output" when all
 *     are NULL.
 * Argument checks before any HIP call: ndim outside 3 .. 13, m outside 1 .. 8, C negative, a bad kind or parameter: RC_EINVAL;
 * C = 0: RC_OK, nothing done; state_dev (or another required pointer) NULL: RC_EINVAL.  Enqueue-only: device pointers, launched on
 * `stream`, no allocation, no synchronisation.  One lane per row, no atomics: same inputs, same bits. */
long long rc_lbfgs_state_len(long long C, int ndim, int m);
int rc_lbfgs_init_f64_async(int device, void* stream, int ndim, int m, long long C, const double* x0_dev, const double* mask_dev,
                            double* state_dev, double* trial_dev);
int rc_lbfgs_advance_f64_async(int device, void* stream, int ndim, int m, long long C, int kind, double lam,
                               const double* row_a_dev, const double* row_b_dev, double c1, double gtol, double ftol,
                               long long maxiter, long long maxback, double* state_dev, double* trial_dev);
int rc_lbfgs_result_f64_async(int device, void* stream, int ndim, int m, long long C, const double* state_dev, double* x_out_dev,
                              double* f_out_dev, double* g_out_dev, int* status_out_dev, long long* iters_out_dev,
                              long long* evals_out_dev);

/* (ABI 14) The BOXED variant of the batched L-BFGS: box bounds lo <= x <= hi per variable and row, by projected steps.  The same
 * state (rc_lbfgs_state_len, layout unchanged: nothing new is stored), the same trial_dev and NaN-row rule, the same kinds,
 * parameters and statuses, and rc_lbfgs_result_f64_async reads the result; the unbounded entries above are untouched (their
 * kernels, arithmetic and bits).  A state started by rc_lbfgs_init_box_f64_async is advanced by rc_lbfgs_advance_box_f64_async only.
 *     lo_dev, hi_dev  [C][ndim] like x0_dev, both required (NULL: RC_EINVAL before any HIP call); -inf / +inf per entry for a side
 *                     without a bound.  They are inputs, not state: hand the SAME two arrays to init and to every advance.
 * With P(v) = v < lo ? lo : (v > hi ? hi : v) (a NaN stays a NaN), the rules that differ from the unbounded machine (the
 * definition is again code-robchar_amd/lbfgs.py, the same bit rules):
 *     start      x0 <- P(x0), masked variables included; a row with a NaN bound or lo_i > hi_i is done at once with status 5
 *     accept     s = trial - x, gs = g.s: accepted iff f_trial is finite and gs < 0 and f_trial <= f + c1 gs
 *     pair       s is the projected step, y = g_trial - g; the store rule is unchanged
 *     status 1   max_i |x_i - P(x - g)_i| <= gtol (the projected gradient of L-BFGS-B)
 *     direction  at every new direction the active set A_i = (x_i <= lo_i and g_i > 0) or (x_i >= hi_i and g_i < 0) is recomputed;
 *                the two-loop recursion starts from g with the A entries 0, the A entries of its result are set to 0, and it is
 *                taken iff a pair is stored and g.d < 0; otherwise steepest descent along -g with the A entries 0 (first step
 *                min(1, 1 / |that vector|_2)) and the history is dropped
 *     trial      P(x + t d), on a new direction and after every halving; reject, maxback, the one reset and status 4 as above
 * Every trial point and every iterate lies inside the box exactly, and an accepted value is never above its predecessor.
 * Not L-BFGS-B: no Cauchy point, no subspace minimisation.  Argument checks, C = 0 and the enqueue-only contract as for ABI 13. */
int rc_lbfgs_init_box_f64_async(int device, void* stream, int ndim, int m, long long C, const double* x0_dev, const double* mask_dev,
                                const double* lo_dev, const double* hi_dev, double* state_dev, double* trial_dev);
int rc_lbfgs_advance_box_f64_async(int device, void* stream, int ndim, int m, long long C, int kind, double lam,
                                   const double* row_a_dev, const double* row_b_dev, const double* lo_dev, const double* hi_dev,
                                   double c1, double gtol, double ftol, long long maxiter, long long maxback,
                                   double* state_dev, double* trial_dev);

/* (ABI 15) Bootstrap of the per-controller metrics, resampled on the device: B replicates of every row of fid [C][K], each a
 * resample of the row's K values with replacement, and their summary - a per-metric error bar from the samples already there.
 * The definition is code-robchar_amd/bootstrap.py (NumPy).
 * Index stream: Philox4x32-10 as in rc_draws_philox_f64_async, key = seed, counter high words 0.  With Q = ceil(K / 4), draw t
 * (0 <= t < K) of replicate b of row c is output word (t & 3) of counter   offset + (c B + b) Q + (t >> 2),   and
 *     idx = (word * K) >> 32.
 * No rejection step: the bias, below K / 2^32, is part of the definition.  Row c of a C-row call equals row 0 of a one-row call
 * with offset + c B Q.
 * With m = the row's mean (fixed summation order), f the K gathered values and g = f - m:   S1 = sum g,  S2 = sum g^2,
 *     rim1 = 1 - (m + S1 / K),   std = sqrt(max(0, S2 / K - (S1 / K)^2))  (population),   min = min f,
 *     q[i] = #{f >= q_thresholds[i]} / K        (signs of rc_reduce_f64: q and min positive).
 * A row holding any NaN gives NaN in every output.  One wave owns one replicate and its summation order depends on K alone: same
 * inputs, same bits, on either route and however the replicates are spread over workgroups.  No atomics.
 *     rep_out     [M][C][B], M = 3 + nq in the order rim1, std, min, q[0 .. nq)         optional (NULL = not wanted)
 *     summary_out [M][4][C]: over the B replicates of a metric and row, their mean, their standard error (std with ddof = 1;
 *                 NaN for B = 1) and the order statistics of ranks rank_lo and rank_hi (0-based, ascending)        optional
 * For a two-sided interval at level conf take a = (1 - conf) / 2, rank_lo = floor(a (B - 1)), rank_hi = ceil((1 - a) (B - 1)).
 * route: 0 = by K, 1 = the row is staged once per workgroup into LDS and resampled from there (K <= 18432: 144 KiB of a CU's
 * 160 KiB), 2 = gathered from global memory (any K).  The routes give the same bits.
 * Argument checks before any HIP call, RC_EINVAL with a message: C negative; K < 1 or above 2^31 - 1; B < 1 or above 16384 (the
 * row sort behind the summary); nq outside [0, 8], or q_thresholds NULL with nq > 0; ranks outside 0 <= rank_lo <= rank_hi < B;
 * route outside 0 .. 2, or route 1 with K above 18432; offset + C B Q wrapping 2^64; fid NULL with C > 0.  C = 0: RC_OK, nothing
 * written.
 * _async: enqueue-only on `stream`, device pointers (q_thresholds is a HOST array, read before the call returns); its workspace
 * (the sorted replicates, and the replicates when rep_out is NULL) is allocated and released in stream order.  The blocking
 * entry takes host or device arrays. */
int rc_bootstrap_metrics_f64_async(int device, void* stream, const double* fid_dev, long long C, long long K, long long B,
                                   unsigned long long seed, unsigned long long offset, const double* q_thresholds, int nq,
                                   long long rank_lo, long long rank_hi, int route, double* rep_out_dev, double* summary_out_dev);
int rc_bootstrap_metrics_f64(int device, const double* fid, long long C, long long K, long long B, unsigned long long seed,
                             unsigned long long offset, const double* q_thresholds, int nq, long long rank_lo, long long rank_hi,
                             int route, double* rep_out, double* summary_out);

/* (ABI 18) Pairwise Wasserstein distances between fidelity rows: for rows a, b of equal length K, each sorted ascending,
 *     W_1 = (1/K) sum_k |a_(k) - b_(k)|,      W_2 = sqrt((1/K) sum_k (a_(k) - b_(k))^2),
 * the exact p-Wasserstein distance between the two empirical distributions (a row of ones as b gives RIM_p).  p = 1 or 2.
 * The definition is code-robchar_amd/wasserstein.py (NumPy, math.fsum).
 *     a [CA][K], b [CB][K]   row-major, every row sorted ascending (what rc_reduce_f64's sorted_out holds)
 *     out [CA][CB]           out[i][j] = W_p(a_i, b_j)
 * b = NULL: the matrix of a against itself, out [CA][CA]; CB is then ignored, whatever it holds.  Only tiles on or above the
 * diagonal are computed and each is written to both places: out equals its transpose bit for bit, and the diagonal of a NaN-free
 * row is exactly 0.
 * Arithmetic: d = a - b, then acc + |d| (p = 1) or fma(d, d, acc) (p = 2) - never sum a^2 + sum b^2 - 2 sum a b, which cancels for
 * close rows; one IEEE division by K, the correctly rounded square root.  A row holding any NaN gives NaN in its whole row and
 * column by ordinary propagation (no min / max anywhere).  The K terms are summed in a fixed order that depends on K alone (in
 * order inside chunks of 256, the chunk sums in order inside blocks of 1024, those inside blocks of 4096, those in order), so an
 * element's bits depend on its two rows, K and p only: not on CA, CB, the position of the rows, the mode, or how the launch
 * spreads K over workgroups.  No atomics: when K is split, the partial sums go to a scratch buffer allocated and released in stream
 * order and a finishing launch adds them in that order.
 * Argument checks before any HIP call, RC_EINVAL with a message: p outside {1, 2}; CA, K or (with b given) CB negative.  Then CA,
 * K or (with b given) CB equal to 0: RC_OK, nothing written.  Then a or out NULL: RC_EINVAL; more than 2^31 - 1 rows: RC_EINVAL.
 * _async: enqueue-only on `stream`, device pointers, sorted rows are a precondition; no synchronisation.  The blocking entry
 * takes host or device arrays; with presorted = 0 it sorts the rows first (the row sort of rc_reduce_f64), leaving a and b as
 * they are.  Timing: DESIGN.md. */
int rc_wasserstein_matrix_f64_async(int device, void* stream, int p, const double* a_sorted_dev, long long CA,
                                    const double* b_sorted_dev /* NULL: B = A, symmetric */, long long CB, long long K,
                                    double* out_dev /* [CA][CB], or [CA][CA] */);
int rc_wasserstein_matrix_f64(int device, int p, const double* a, long long CA, const double* b, long long CB, long long K,
                              int presorted, double* out);

/* (ABI 6) 1 when the kernel above is the faster of the two bit-identical routes for this geometry (N <= 13, or N = 14 with
 * {in, out} = {0, N-1}), else 0; 0 everywhere when ROBCHAR_PHILOX_FUSED=0 is in the environment (read per call).  The ONE
 * copy of that rule: the sharded entries below and the Python layer (backend.philox_fused_pays) both ask it. */
int rc_philox_fused_pays(int N, int in, int out);

/* (ABI 16) Fidelity on a grid of readout times from ONE eigen decomposition per sample.  Chain topology, N = 2 .. RC_MAX_NSPIN_FAST,
 * any (in, out).  The grid has M times, 1 <= M <= RC_MAX_TIMES; for controller row c (time entry T_c, signed as stored)
 *     t_cj = | T_c tscale[j] + tshift[j] |        product rounded first, sum second (no fused multiply-add), absolute value last:
 *                                                  NumPy's np.abs(T[:, None] * tscale + tshift), bit for bit
 *     F_j(c, k) = |<out| exp(-i H_ck t_cj) |in>|^2,   H_ck as in rc_mc_fidelity_f64.
 * tscale, tshift: [M] each, NULL = all 1 / all 0.  Outputs, each optional (NULL = not wanted; all three NULL: RC_EINVAL "no output"):
 *     fid_out  [M][C][K]   M slabs, each an ordinary [C][K] fidelity tensor (what rc_reduce_f64, rc_bootstrap_metrics_f64,
 *                          rc_tail_select_f64_async take); slab j is bit for bit what kernel = RC_KERNEL_TRIDIAG_QL gives for
 *                          controllers whose time entry is t_cj
 *     wsum_out [C][K]      acc = weights[0] F_0;  acc = fma(weights[j], F_j, acc), j = 1 .. M - 1: fixed order.  Needs weights [M]
 *                          (NULL with wsum_out set: RC_EINVAL)
 *     fmin_out [C][K]      min_j F_j, taken in the order of j
 * A controller row holding a NaN gives NaN in every output and its draws are not read.  One all-fp64 implicit QL with the
 * eigenvector rows `in` and `out` per sample (no condition on eigenvalue gaps or cut bonds), then N - 1 table-driven sines and
 * cosines per time.  Their argument must stay inside the table routine's domain:  |t_cj (lambda_k - lambda_0)| < 2.1e8  for every
 * eigenvalue lambda_k of H_ck (as for every register-resident chain kernel at the row's own T); beyond it the result is undefined.
 * A sample whose QL runs into its sweep cap (observed for H = 0 exactly, nothing else) takes a textbook per-sample routine,
 * counted per tile in rc_stats_times_general_tiles.
 * Argument checks before any HIP call: N, in, out, C, K as in rc_mc_fidelity_f64 (RC_EINVAL); N > RC_MAX_NSPIN_FAST or ring != 0:
 * RC_ENOSUP; M outside 1 .. RC_MAX_TIMES, no output, wsum_out without weights, draws_ctrl_stride overlapping controllers:
 * RC_EINVAL; C or K = 0: RC_OK, nothing written; controllers or draws NULL: RC_EINVAL.
 * draws_ctrl_stride: K*N*3 (or negative) for one draw block per controller, 0 for ONE set of K draws shared by every controller.
 * _async: enqueue-only - device pointers for controllers, draws, tscale, tshift, weights and the outputs; one kernel launch on
 * `stream`, no allocation, no synchronisation, capturable into a graph.  The blocking entry takes host or device arrays. */
#define RC_MAX_TIMES 64
int rc_mc_fidelity_times_f64_async(int device, void* stream, int N, int in, int out, const double* h0_diag, const double* h0_offdiag,
                                   int ring, const double* controllers_dev, const double* draws_dev, long long draws_ctrl_stride,
                                   long long C, long long K, int M, const double* tscale_dev, const double* tshift_dev,
                                   const double* weights_dev, double* fid_out_dev, double* wsum_out_dev, double* fmin_out_dev);
int rc_mc_fidelity_times_f64(int device, int N, int in, int out, const double* h0_diag, const double* h0_offdiag, int ring,
                             const double* controllers, const double* draws, long long draws_ctrl_stride, long long C, long long K,
                             int M, const double* tscale, const double* tshift, const double* weights, double* fid_out,
                             double* wsum_out, double* fmin_out);
/* The same with the counter-based draws generated inside the kernel: sample (c, k), site i, slot s is element
 *     offset + ((c K + k) N + i) 3 + s      of stream `seed` (rc_draws_philox_f64_async), scaled by sigma_rows_dev[c], or by `sigma`
 * when sigma_rows_dev is NULL (then a negative or non-finite sigma is RC_EINVAL).  Every output is bit-identical to
 * rc_draws_philox_f64_async into a [C][K][N][3] tensor followed by rc_mc_fidelity_times_f64_async.  Enqueue-only. */
int rc_mc_fidelity_times_philox_f64_async(int device, void* stream, int N, int in, int out, const double* h0_diag,
                                          const double* h0_offdiag, int ring, const double* controllers_dev, unsigned long long seed,
                                          unsigned long long offset, double sigma, const double* sigma_rows_dev, long long C,
                                          long long K, int M, const double* tscale_dev, const double* tshift_dev,
                                          const double* weights_dev, double* fid_out_dev, double* wsum_out_dev, double* fmin_out_dev);
/* Diagnostic (ABI 16): the counter of rc_stats_grad_general_tiles for the two readout-time kernels. */
long long rc_stats_times_general_tiles(int device, int reset);

/* (ABI 17) rc_mc_fidelity_grad_philox_f64_async ON A GRID OF READOUT TIMES, from ONE eigen decomposition per sample: the weighted
 * fidelity over the grid and its gradient with respect to the controller row - the objective 1 - E_draws E_delta F(T + delta) of a
 * controller under readout-time jitter, and its moment sums, in one launch.  The grid is that of rc_mc_fidelity_times_f64_async:
 * M times, 1 <= M <= RC_MAX_TIMES, tscale_dev [M] and tshift_dev [M] (NULL = all 1 / all 0), weights_dev [M] (required).  For
 * controller row c with time entry T_c (signed, as stored)
 *     u_cj = T_c tscale_j + tshift_j        (the product rounded first, the sum second; |u_cj| is the t_cj of the times entries),
 *     W(c, k)   = sum_j w_j F_j(c, k),      dW/dx_l = sum_j w_j dF_j/dx_l           for the N biases,
 *     dW/dx_N   = sum_j w_j tscale_j sgn(u_cj) F_j'(|u_cj|)                         (a time with u_cj = 0 contributes 0),
 * the grid and the weights being constants of the objective.  Per time the sample's F_j and gradient are those of
 * rc_mc_fidelity_grad_philox_f64_async for a controller whose time entry is u_cj, the time entry then multiplied by tscale_j
 * (rounded once); every sum is  acc = w_0 v_0; acc = fma(w_j, v_j, acc), j = 1 .. M - 1.  So wfid_out and wgrad_out are BIT FOR BIT
 * what M launches of that entry, the scaling of the time column and that fma sequence give, and with M = 1, the unit grid and
 * w = 1 all four outputs are that entry's bits.
 * Outputs, each optional (NULL = not wanted; all four NULL: RC_EINVAL):
 *     wfid_out [C][K] = W, wgrad_out [C][K][N+1] = dW/dx, mean_out [C][N+2] = (mean W, mean dW/dx),
 *     moment_out [C][N+2] = (mean W^2, mean W dW/dx_0 .. mean W dW/dx_N): as in rc_mc_fidelity_grad_philox_f64_async with F
 *     replaced by W (rc_lbfgs_advance_f64_async takes the two rows as they are).
 * Stream conventions (shared_draws), sigma / sigma_rows_dev, NaN rows, empty batches (C = 0 or K = 0: RC_OK, nothing written), the
 * scratch behind mean_out / moment_out and the sweep-cap counter (rc_stats_grad_general_tiles): as there.  Argument checks before any
 * HIP call: N, in, out, C, K as there (N > RC_MAX_NSPIN_GRAD: RC_ENOSUP, "N <= 12"); M outside 1 .. RC_MAX_TIMES, weights_dev NULL,
 * no output: RC_EINVAL; sigma negative or non-finite without sigma_rows_dev: RC_EINVAL.  Enqueue-only: device pointers (the grid
 * included), launched on `stream`.  Timing against M launches of the single-time entry: DESIGN.md. */
int rc_mc_fidelity_grad_times_philox_f64_async(int device, void* stream, int N, int in, int out, const double* h0_diag,
                                               const double* h0_offdiag, const double* controllers_dev, unsigned long long seed,
                                               unsigned long long offset, double sigma, const double* sigma_rows_dev,
                                               int shared_draws, long long C, long long K, int M, const double* tscale_dev,
                                               const double* tshift_dev, const double* weights_dev, double* wfid_out_dev,
                                               double* wgrad_out_dev, double* mean_out_dev, double* moment_out_dev);


/* Non-Hermitian variant: `diag_imag_dev` [C][K][N] (or NULL) is added to the diagonal as an IMAGINARY part,
 * H[i][i] += 1j * diag_imag.  Chains up to N = 12: a lane-per-sample complex symmetric QL kernel (the couplings stay
 * Hermitian pairs, so the diagonal gauge makes them real and leaves a complex symmetric tridiagonal matrix), with the dense
 * Pade-expm kernel (RC_KERNEL_EXPM's) as repair pass over the samples it marks; rings and N > 12: the expm kernel for every
 * sample (also when RC_NH_EXPM_ONLY=1 is in the environment - the cross-check).  This is the draw layout of the reference's
 * `directional_perturbation` (noise_model.py:150-201): a sample perturbs ONE element pair; a bond direction maps
 * onto (g1, g2) of the ordinary draws, a diagonal direction (i,i) ends up as a - ib on the diagonal because the
 * second assignment (noise_model.py:198-199) overwrites the first: g0_i = a, diag_imag_i = -b. */
int rc_mc_fidelity_nh_f64_async(int device, void* stream, int N, int in, int out,
                                const double* h0_diag, const double* h0_offdiag, int ring,
                                const double* controllers_dev, const double* draws_dev,
                                const double* diag_imag_dev, long long C, long long K, double* fid_out_dev);

/* `directional_perturbation` (noise_model.py:150-201) evaluated straight from what its RNG consumption leaves per sample
 * (ABI 5): idx_dev [C][K] (int32) = the direction index `np.random.randint(0, len(directions))` drew, ab_dev [C][K][2] = the
 * two normals of `rng(size=2)`, already scaled by sigma - exactly what rc_directional_draws_legacy_dev writes.  The sample
 * perturbs ONE element pair: z[p,q] = a + ib, z[q,p] = a - ib with (p, q) = directions[idx] in the reference's list order
 * [(0,0), (N-1,N-1), (d,d-1), (d,d), (d,d+1) for d = 1..N-2, (0,1), (1,0), (N-2,N-1), (N-1,N-2)]; for p = q the second
 * assignment wins (H[p][p] += a - ib: non-Hermitian).  No (C, K, N, 3) draw tensor exists: the samples are partitioned by
 * class on the device and evaluated lane per sample - bond directions by the real tridiagonal routes, diagonal directions by
 * the complex symmetric QL route, whatever neither settles by the Pade-expm kernel.  Chain topology, N <= 12 (RC_ENOSUP
 * otherwise: build the dense layout and call rc_mc_fidelity_nh_f64_async).  Enqueue-only; the workspace (8 bytes per
 * sample) is allocated and released in stream order. */
int rc_mc_fidelity_directional_f64_async(int device, void* stream, int N, int in, int out,
                                         const double* h0_diag, const double* h0_offdiag, int ring,
                                         const double* controllers_dev, const int* idx_dev, const double* ab_dev,
                                         long long C, long long K, double* fid_out_dev);

/* Per-controller reductions over K.  Outputs are variant-major with 3 variants in the order
 *   0: centre  F          1: " upper"  clip(F - dkw_eps, 0, 1)        2: " lower"  clip(F + dkw_eps, 0, 1)
 * (naming of mcsim.py:484-485).  Shapes: rim1/std_/minf [3][C];  q [3][nq][C] = fraction of samples >=
 * q_thresholds[j] (the reference stores the NEGATED value; signs are applied by the host layer).
 * std_ is the population standard deviation (np.std).  A row holding ANY NaN - all of it (a padded controller) or a single
 * value - gives NaN in rim1 / std_ / minf of all three variants.  Its q is the count of the non-NaN values >= threshold over K
 * (the reference's Q, where NaN counts as below): 0 for a whole-NaN row, not for a row with some NaN.  Inside the two shifted
 * variants a NaN is clamped to 0, so there - unlike np.clip, which keeps it - it counts against a threshold <= 0.
 * sorted_out: NULL, or [C][K] receiving each row sorted ascending (a row holding any NaN is copied through unchanged); any K (one
 * launch for K <= 16384, a bitonic network with HBM passes above; internal grow-only workspace).
 * Any output pointer may be NULL to skip it.  nq <= 8.  q_thresholds is a HOST pointer.
 * Summation order: fixed per (K, route) - bitwise reproducible from run to run.  The kernel is chosen by K (one workgroup of
 * 128 / 256 / 512 threads per row for K <= 4096 / 8192 / above); for K <= 2048 also by C (C >= 64: one wave per row), so below
 * that length the last bits of mean / std of a row may depend on how many rows are reduced together, above it they do not;
 * for 8192 < K <= 10240 also by the overlap hint of rc_reduce_ex_f64_async (this blocking entry: RC_REDUCE_STANDALONE). */
int rc_reduce_f64(int device, const double* fid, long long C, long long K,
                  const double* q_thresholds, int nq, double dkw_eps,
                  double* rim1, double* std_, double* minf, double* q, double* sorted_out);

int rc_reduce_f64_async(int device, void* stream, const double* fid_dev, long long C, long long K,
                        const double* q_thresholds, int nq, double dkw_eps,
                        double* rim1_dev, double* std_dev, double* minf_dev, double* q_dev,
                        double* sorted_out_dev);

/* (ABI 6) The same with a hint about what runs BESIDE the reduction.  flags = 0: rc_reduce_f64_async (a caller that overlaps
 * the reduction with fidelity launches on another stream: the latency-bound 512-thread route for rows of 8193 .. 10 240 values
 * fills issue slots those kernels leave idle).  RC_REDUCE_STANDALONE: nothing overlaps it - rows of that length go through 256
 * threads x 40 register-cached values, five rows in flight per CU instead of two (11 000 rows of 10 000 values: 440 -> 208 us;
 * 1 000 rows: 46 -> 29.5 us).  The blocking rc_reduce_f64 and the multi-device entries always reduce standalone.  The flag picks
 * the route and with it the summation order of rows of THAT length: mean / std may differ in the last bits between the two. */
#define RC_REDUCE_STANDALONE 1
int rc_reduce_ex_f64_async(int device, void* stream, const double* fid_dev, long long C, long long K,
                           const double* q_thresholds, int nq, double dkw_eps,
                           double* rim1_dev, double* std_dev, double* minf_dev, double* q_dev,
                           double* sorted_out_dev, int flags);

/* p-RIM per controller: out[c] = (mean_k (1 - fid[c][k])^p)^(1/p), p > 0.  fid [C][K], out [C]. */
int rc_rim_p_f64(int device, const double* fid, long long C, long long K, double p, double* out);
int rc_rim_p_f64_async(int device, void* stream, const double* fid_dev, long long C, long long K, double p,
                       double* out_dev);

/* Counter-based Gaussian draws on the device (Philox4x32-10 + Box-Muller, fp64), for sample spaces too large
 * to draw on the host.  NOT the reference's RNG (the reference uses numpy's legacy MT19937 stream, which the
 * host layer reproduces exactly); provided for scale, with parity checked by regenerating the same elements on
 * the host (oracle/philox_host.py).  out[i] = scale * z(seed, offset + i), i < n: the stream is indexed by
 * element, so any slice - e.g. one rank's controller block - can be generated independently. */
int rc_draws_philox_f64(int device, unsigned long long seed, unsigned long long offset, long long n, double scale,
                        double* out);
int rc_draws_philox_f64_async(int device, void* stream, unsigned long long seed, unsigned long long offset,
                              long long n, double scale, double* out_dev);

/* (ABI 19) Randomised quasi-Monte Carlo: scrambled Sobol points and their normals.  code-robchar_amd/sobol.py (NumPy only) is the
 * DEFINITION; the device reproduces its integer points bit for bit and its normals to a few ulp.
 *   point    dimension d, index n (0 <= n < 2^32), direction numbers v[d][0..31] (uint32, bit 31 = first binary digit):
 *            x = XOR over the set bits j of gray(n) = n ^ (n >> 1) of v[d][j], then x ^= shift[d]   (SciPy's and torch's order)
 *   normal   u = (x + 0.5) 2^-32 in (0, 1);  z = Phi^-1(u) by Wichura's AS 241 (PPND16), |z| <= 6.34, z(~x) == -z(x) exactly;
 *            draw = fl(sigma z), one rounded product
 *   samples  sample k of controller row c belongs to replicate r = k / P and is point n = skip + (k mod P) of that replicate;
 *            tables dirnum[R][D][32] and shift[Cs][R][D], the shifts read at row c when shift_cstride = R D and at row 0 when
 *            shift_cstride = 0 (common random numbers across controllers)
 *   contract 1 <= D <= RC_SOBOL_MAX_DIM, R >= 1, K <= R P, skip % 64 == 0, P % 64 == 0 whenever R > 1, skip + min(P, K) <= 2^32,
 *            shift_cstride 0 or R D; anything else is RC_EINVAL.  C == 0 or K == 0: RC_OK, nothing written.
 * rc_sobol_dirnum_u32: host only, no HIP call - the unscrambled Joe-Kuo table out_host[D][32] of the first D dimensions (a C client
 * scrambles it as sobol.py's `scramble` does, or uses it as it is with zero shifts).
 * rc_draws_sobol_f64_async: draws_out_dev [C][K][D] fp64 = sigma_c z (sigma_rows_dev[c], or `sigma` when that is NULL) and
 * bits_out_dev [C][K][D] uint32 = the points x; either may be NULL, not both.  For D = 3 N the draws are the [C][K][N][3] tensor
 * every entry that reads draws takes.  No atomics: same inputs, same bits.  rc_draws_sobol_f64: the blocking twin, host or device
 * pointers. */
int rc_sobol_dirnum_u32(int D, unsigned int* out_host);
int rc_draws_sobol_f64_async(int device, void* stream, int D, const unsigned int* dirnum_dev, const unsigned int* shift_dev,
                             long long shift_cstride, int R, long long P, long long skip, double sigma, const double* sigma_rows_dev,
                             long long C, long long K, double* draws_out_dev, unsigned int* bits_out_dev);
int rc_draws_sobol_f64(int device, int D, const unsigned int* dirnum, const unsigned int* shift, long long shift_cstride, int R,
                       long long P, long long skip, double sigma, const double* sigma_rows, long long C, long long K,
                       double* draws_out, unsigned int* bits_out);
/* The chain fidelity kernel with the Sobol normals generated inside it (D = 3 N, dimension 3 i + s for site i, slot s): no draw
 * tensor.  BIT-IDENTICAL to rc_draws_sobol_f64_async followed by rc_mc_fidelity_f64_async(RC_KERNEL_AUTO) on that tensor.  Chain
 * topology, N = 2 .. RC_MAX_NSPIN_SOBOL, RC_KERNEL_AUTO / RC_KERNEL_TRIDIAG_ADJ; everything else is RC_ENOSUP (use the two-kernel
 * route).  A NaN controller row gives NaN. */
int rc_mc_fidelity_sobol_f64_async(int device, void* stream, int kernel, int N, int in, int out, const double* h0_diag,
                                   const double* h0_offdiag, const double* controllers_dev, const unsigned int* dirnum_dev,
                                   const unsigned int* shift_dev, long long shift_cstride, int R, long long P, long long skip,
                                   double sigma, const double* sigma_rows_dev, long long C, long long K, double* fid_out_dev);

/* (ABI 20) Variance-based noise sensitivity indices by the pick-freeze scheme.  code-robchar_amd/variance_indices.py (NumPy only)
 * is the DEFINITION.  Coordinate j = 3 i + s of a sample is slot s of site i in the draw layout [N][3]; a group is a uint64 mask
 * over the 3 N coordinates (bits >= 3 N must be zero; bits 1 and 2 - the dropped g1_0, g2_0 - are allowed and change nothing).
 * Per sample (c, k) two draw vectors: a = elements offset_a + ((c K + k) N + i) 3 + s of stream `seed` scaled by sigma (exactly
 * the draws of rc_mc_fidelity_philox_f64_async), b = the same at offset_b; the two ranges [offset, offset + C K 3N) must be
 * disjoint (distances modulo 2^64: a wrapping offset is legal).  Hybrid h_g = b where groups[g] has the bit, a elsewhere - a copy
 * of bits -; fA = F(a), fB = F(b), f_g = F(h_g).
 *   fid_out_dev  [G + 2][C][K] or NULL: slab 0 = fA, 1 = fB, 2 + g = f_g.  Slab 0 is BIT-IDENTICAL to
 *                rc_mc_fidelity_philox_f64_async(seed, offset_a), slab 1 to the same at offset_b, slab 2 + g to
 *                rc_mc_fidelity_f64_async(RC_KERNEL_AUTO) on the materialised hybrid tensor.
 *   mean_out_dev [C][3 + 2 G] or NULL: the means over k of fA, fB, D = (fA - fB)^2 and, per group, T_g = (fA - f_g)^2 and
 *                U_g = (fB - f_g)^2 (Jansen's estimators: a difference rounded once, a square rounded once, sums of non-negative
 *                terms in a fixed order - no atomics: same inputs, same bits, with or without fid_out_dev).  Var F = D / 2,
 *                total-order index T_g / D, first-order index 1 - U_g / D.  A NaN controller row gives NaN everywhere.
 * It replaces, for G groups, two rc_draws_philox_f64_async launches, G selections over [C][K][N][3] tensors, G + 2
 * rc_mc_fidelity_f64_async launches and 2 G + 1 elementwise reductions; no draw tensor exists.  `groups` is a HOST array read
 * during the call (no device copy, nothing to keep alive).  sigma / sigma_rows_dev as in rc_mc_fidelity_philox_f64_async.
 * Enqueue-only: never synchronises.  Refused before any HIP call: N outside 2 .. RC_MAX_NSPIN_PICKFREEZE or a kernel other than
 * RC_KERNEL_AUTO / RC_KERNEL_TRIDIAG_ADJ (RC_ENOSUP), G outside [0, RC_PICKFREEZE_MAX_GROUPS], a mask with a bit >= 3 N,
 * overlapping element ranges, both outputs NULL, NULL controllers with C > 0, too many tiles (RC_EINVAL).  C == 0 or K == 0: RC_OK
 * behind the contract, nothing written.  The repair routes count into rc_stats_general_tiles / rc_stats_polish_tiles. */
int rc_mc_fidelity_pickfreeze_philox_f64_async(int device, void* stream, int kernel, int N, int in, int out, const double* h0_diag,
                                               const double* h0_offdiag, const double* controllers_dev, unsigned long long seed,
                                               unsigned long long offset_a, unsigned long long offset_b, double sigma,
                                               const double* sigma_rows_dev, const unsigned long long* groups, int G, long long C,
                                               long long K, double* fid_out_dev, double* mean_out_dev);

/* The reference's OWN random stream on the device: NumPy's legacy `RandomState` normal generator (MT19937 + polar
 * Box-Muller, what `np.random.normal` at noise_model.py:114-115 draws from), continued from `state` - the caller's
 * `np.random.get_state()`: key[624], pos, has_gauss, cached_gaussian - and left exactly where NumPy would leave it after
 * the same number of draws (uint32 stream, attempt boundaries, cached value: bit-identical; the normals themselves are NumPy's
 * bit for bit where rc_legacy_log_is_host_exact() says so - round 5: the device evaluates glibc's log operation for operation -
 * and within a few ulp otherwise).  The stream is cut into `n_periods` periods of `period` normals; the
 * first `skip` of every period are consumed but dropped (the burned draw of `rng(scale=sigma)`, mcsim.py:425), the others
 * are written contiguously to out_dev[p * (period - skip) ...] multiplied by scales[p] (HOST pointer, [n_periods]).
 * One call = all sigma levels of an algorithm: period = 1 + C*K*3N, skip = 1, scales = the levels.
 * Blocking with respect to `state` (updated on return); the output is produced on `stream`. */
typedef struct rc_mt19937_state {
    unsigned int key[624];
    int pos;
    int has_gauss;
    double gauss;
} rc_mt19937_state;
int rc_draws_legacy_f64(int device, void* stream, rc_mt19937_state* state, long long n_periods, long long period,
                        long long skip, const double* scales, double* out_dev);

/* (ABI 6) The normals of the two device-side legacy entries (rc_draws_legacy_f64, rc_directional_draws_legacy_dev) are NumPy's
 * BIT FOR BIT when the C library's log() is the routine the device restates operation for operation: glibc >= 2.28's
 * table-driven double log in the FMA build its resolver selects on x86-64 with FMA + AVX2 (legacy_rng_core.h: log_glibc_fma;
 * division and square root are correctly rounded on both sides).  1 = verified on this host (2^17 arguments against log()
 * itself, once per process); 0 = another libm: state and attempt boundaries are still exact, the normals may differ from
 * NumPy's in the last bits - a caller that needs identical DRAWS then draws on the host (the Python layer does so by itself). */
int rc_legacy_log_is_host_exact(void);

/* Host-side (CPU) emulation of the RNG consumption of `directional_perturbation.perturbation()` (noise_model.py:183-189)
 * on NumPy's legacy stream `state` (updated): per sample `np.random.randint(0, ndir)` then two legacy normals scaled by
 * sigma.  idx_out [n], ab_out [n][2].  Bit-identical to NumPy (indices, normals, state); ~100x the Python loop. */
int rc_directional_draws_legacy(rc_mt19937_state* state, long long n, int ndir, double sigma, int* idx_out, double* ab_out);

/* The same consumption pattern with the work on the GPU (ABI 4): raw MT19937 words from jump-ahead sub-streams, one
 * kernel finds for EVERY word position how many words a sample starting there would consume, the chain of sample starts
 * through that byte array - the only sequential step - is followed ON THE DEVICE (round 4: "entry offset -> exit offset"
 * maps of 2048-position blocks composed over superblocks, a few hundred dependent LDS reads per level; the host's own walk
 * of round 3 - 16 MB over PCIe, ~2 ns per sample - remains as the fallback for what the device walk does not follow: a
 * sample longer than 64 words across a block boundary), and one kernel emits index + the two normals per sample.  idx_dev
 * [n] (int32) and ab_dev [n][2] (fp64) are DEVICE pointers, filled in stream order on `stream`; `state` is updated on
 * return (the call synchronises the stream once, for a 2.5 KB state record).  Indices and generator state bit-identical to
 * NumPy's, normals within a few ulp (the device's ln), as for rc_draws_legacy_f64.  Environment, read per call (test / A/B
 * knob): RC_DIR_WALK=host forces the host walk, RC_DIR_WALK=fallback runs the device pass and then the host walk. */
int rc_directional_draws_legacy_dev(int device, void* stream, rc_mt19937_state* state, long long n, int ndir, double sigma,
                                    int* idx_dev, double* ab_dev);

/* Diagnostic: number of 64-sample tiles of the chain kernels in which at least one sample left the wave-wide fast path
 * and was repaired per sample on `device` since the last reset; synchronises the device.  A sample is repaired when it has
 * a degenerate eigenvalue pair (closer than 1e-12 of the spectral scale for the end-to-end weights, 4e-6 for the general
 * adjugate weights), when the a-posteriori sum-rule guard of the general adjugate weights rejects it, on the
 * sweep cap, or on overflow.  Rare but not impossible on random workloads - measured on the BASELINE shapes (GPU suite,
 * rounds 3 / 4): 0 tiles for configs 2 and 3 (N launches of 15 700 tiles each, every `out`), ~150-200 for config 5's ten
 * launches, 3 of config 4's 1 563 000; the tests bound it at ~10x those counts (tests/test_gpu_fullsize.py,
 * tests/test_gpu_chain.py).  One such tile costs a 1e6-evaluation launch +0.3 %.  Ring route: repaired WAVES of 64 listed
 * samples (one per 1e6-evaluation launch at N = 7).  Negative on error. */
long long rc_stats_general_tiles(int device, int reset);

/* Diagnostic (ABI 3): tiles of the mixed-precision eigenvalue path (chain kernels, N = 3..13, eigenvalue-only weight modes)
 * in which some sample needed more than the one fp64 step (close eigenvalue pair); such a tile keeps stepping - still
 * on the fast path - and costs ~20 % more.  ~9 % of the tiles of the N = 7 benchmark workload.  Same conventions. */
long long rc_stats_polish_tiles(int device, int reset);

/* Single-process multi-device entry points (the reference's only parallel construct is the dead
 * multiprocessing.Pool of mcsim.py:451-455).  The C controllers are split into `ndev` contiguous balanced blocks (the
 * first C mod ndev devices get one extra), block r on device devices[r] (devices == NULL: 0 .. ndev-1); one host
 * thread and one stream per device, all devices concurrently; every array is a HOST pointer and results are assembled
 * in the caller's host arrays, so no collective is involved.  Blocking; thread-safe (per-device locks).
 *
 * rc_mc_fidelity_sharded_f64: rc_mc_fidelity_kernel_f64 over several devices - controllers [C][N+1], draws
 *   [C][K][N][3], fid_out [C][K].
 * rc_mc_metrics_sharded_f64: fidelity + the per-controller reductions of rc_reduce_f64 on the devices; only the metric
 *   rows come back (rim1 / std_ / minf [3][C], q [3][nq][C]; any may be NULL) plus, optionally, fid_out [C][K] (NULL =
 *   metrics only: nothing of size C x K crosses PCIe).  draws == NULL: the perturbations are generated on the devices
 *   by the counter-based generator of rc_draws_philox_f64 - sample (c, k), site i, slot s is element
 *   philox_offset + ((c K + k) N + i) 3 + s of stream philox_seed, scaled by sigma - so the result does not depend on
 *   ndev (BASELINE config 4: 2.1e9 draws per level never exist on the host).
 *   (Chain, N <= 13 - and end-to-end pairs at N = 14 -, eigenvalue-only kernels: the draws are generated INSIDE the fidelity
 *   kernel - see rc_mc_fidelity_philox_f64_async -, no draw tensor exists and a chunk is bounded by its fidelities alone; at
 *   larger N generating the tensor first is the faster route, with bit-identical results.)
 * Devices process their block in chunks of <= 4 GiB of draws through a grow-only per-device workspace.  A device may
 * be listed once (RC_ALLOW_DUPLICATE_DEVICES=1 in the environment lifts that for rehearsing the multi-block assembly on a
 * one-GPU box: the blocks then take turns on the device). */
int rc_mc_fidelity_sharded_f64(int ndev, const int* devices, int kernel, int N, int in, int out,
                               const double* h0_diag, const double* h0_offdiag, int ring,
                               const double* controllers, const double* draws, long long C, long long K,
                               double* fid_out);
int rc_mc_metrics_sharded_f64(int ndev, const int* devices, int kernel, int N, int in, int out,
                              const double* h0_diag, const double* h0_offdiag, int ring,
                              const double* controllers, const double* draws,
                              unsigned long long philox_seed, unsigned long long philox_offset, double sigma,
                              long long C, long long K, const double* q_thresholds, int nq, double dkw_eps,
                              double* rim1, double* std_, double* minf, double* q, double* fid_out);

/* (ABI 6) The exchange step over RCCL / xGMI from the C ABI (`rc_comm_init` + a communicator handle; north_star:
 * "an RCCL all-gather over xGMI to reassemble per-controller fidelity vectors") - for an integrator without torch.distributed.
 *   rc_comm_init(ndev, devices, &comm): one process, one RCCL communicator per listed device (ncclCommInitAll; devices == NULL:
 *     0 .. ndev-1; a device may be listed once).  librccl.so is resolved at run time - the copy the process already carries
 *     (PyTorch ships one), else librccl.so.1, opened RTLD_LOCAL | RTLD_DEEPBIND (a process that imports PyTorch AFTERWARDS then
 *     holds two RCCL / rocm_smi pairs; kept out of the global scope they do not share their global objects) - so the library
 *     has no link-time dependency on it; RC_ENOSUP when there is none.
 *   rc_mc_metrics_gathered_f64(comm, ...): rc_mc_metrics_sharded_f64's work - controller blocks, one host thread and one stream
 *     per device, draws from the host or (draws == NULL) from the counter-based stream - but the results stay ON THE DEVICES and
 *     are exchanged there: every device all-gathers its block's metric rows and (fid_dev != NULL) its fidelity slab, in ONE RCCL
 *     group on the devices' streams, so that EVERY device ends with everything:
 *       table_dev[r] (device pointer on devices[r], or table_dev == NULL)  [ndev][NR][Cmax],  NR = 9 + 3 nq rows per block:
 *                    rim1[3], std[3], min[3], q[3][nq] (variant order of rc_reduce_f64), Cmax = ceil(C / ndev) columns of
 *                    which block b fills the first C/ndev (+1 for b < C mod ndev); the rest is padding
 *       fid_dev[r]   (or fid_dev == NULL)  [ndev][Cmax][K], same padding
 *       table_host   (or NULL) [NR][C], fid_host (or NULL; with ndev > 1 it needs fid_dev) [C][K]: unpadded copies from devices[0].
 *     Blocking; the results do not depend on ndev (same partition, same stream elements, per-controller reductions).
 * On this pool only a ONE-device communicator can execute (one GPU per box; RCCL refuses two ranks on one device): the
 * multi-device path is correct by construction and rehearsed with ndev = 1 (tests/test_gpu_multidevice.py). */
typedef struct rc_comm rc_comm;
int rc_comm_init(int ndev, const int* devices, rc_comm** comm_out);
int rc_comm_size(const rc_comm* comm);
int rc_comm_destroy(rc_comm* comm);
int rc_mc_metrics_gathered_f64(rc_comm* comm, int kernel, int N, int in, int out,
                               const double* h0_diag, const double* h0_offdiag, int ring,
                               const double* controllers, const double* draws,
                               unsigned long long philox_seed, unsigned long long philox_offset, double sigma,
                               long long C, long long K, const double* q_thresholds, int nq, double dkw_eps,
                               double* const* table_dev, double* const* fid_dev, double* table_host, double* fid_host);

/* Cached-results layout, host side (no GPU involved).  JSON text of a row-major fp64 array of `ndim` (1..8) dimensions
 * as nested lists, exactly parseable by the reference's `json.load` cache-hit branches (mcsim.py:396-397, :504-506):
 * ", " separators, `NaN` / `Infinity` / `-Infinity` tokens like Python's `json.dump` (mcsim.py:457-459, :501), shortest
 * round-trip digits (every value reads back to the identical double), integral values written with ".0".  Formatted by
 * `nthreads` host threads (<= 0: all).  rc_json_bound_f64 returns an upper bound of the text size in bytes;
 * rc_json_encode_f64 needs `cap` >= that bound and returns the number of bytes written (no terminator), or a
 * negative RC_E* code; rc_json_write_f64 streams the same text to the open file descriptor `fd` (at its current
 * offset) in blocks, without materialising it. */
long long rc_json_bound_f64(int ndim, const long long* shape);
long long rc_json_encode_f64(const double* data, int ndim, const long long* shape, char* out, long long cap,
                             int nthreads);
long long rc_json_write_f64(int fd, const double* data, int ndim, const long long* shape, int nthreads);

/* Process-wide default kernel of rc_mc_fidelity_f64 (initially RC_KERNEL_AUTO).
 *
 * Threading: the blocking entry points serialise on an internal PER-DEVICE lock (calls on different devices run
 * concurrently) and may be called from any thread; the *_async entry points only enqueue work on the caller's stream and
 * keep no shared state (the long-row sort allocates its workspace in stream order, per call); rc_last_error() is
 * thread-local. */
int rc_set_fidelity_kernel(int kernel);

#ifdef __cplusplus
}
#endif
#endif /* ROBCHAR_HIP_H */
