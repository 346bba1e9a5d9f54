"""Noise models of the MC path - API mirror of noise_model.py, evaluated on the GPU.

    noise_function             stateful RNG wrapper: a call merges its kwargs into the stored ones and then
                               draws (noise_model.py:21-46) - so ``rng(scale=s)`` sets sigma AND burns a draw.
    noise_model_base           chain/ring XX Hamiltonian `HH`, one-hot controls `CC`, default Gaussian rng
                               (noise_model.py:71-95, :114-115) and `evaluate_noisy_fidelity` (:98-109).
    structured_perturbation    3N draws per sample in the order (g0_i, g1_i, g2_i) (noise_model.py:122-147).

What differs from the reference is only WHERE the arithmetic runs: a sample is described by its 3N draws
(never by a dense N x N perturbation matrix) and fidelities come from `rc_mc_fidelity_f64`.  The batched
entry `fidelity_batch` draws a whole (C, K, N, 3) tensor with ONE generator call, which consumes numpy's
legacy stream exactly like the reference's 3 N C K scalar calls (same values, same order).
"""
from __future__ import annotations

import numpy as np

from . import backend, lbfgs


class noise_function:
    def __init__(self, generator, **args):
        self.generator = generator
        self.args = args

    def __call__(self, **extraargs):
        self.args.update(extraargs)          # sticky, as in the reference (noise_model.py:42-44)
        return self.generator(**self.args)

    def draw_block(self, shape):
        """`shape` draws with the current arguments WITHOUT making `size` sticky.  Generators that take
        ``size=`` (numpy's do) are called once; anything else is called element by element in C order."""
        try:
            block = self.generator(**{**self.args, "size": tuple(shape)})
            block = np.asarray(block, dtype=np.float64)
            if block.shape == tuple(shape):
                return block
        except TypeError:
            pass
        flat = np.empty(int(np.prod(shape)), dtype=np.float64)
        for i in range(flat.size):
            flat[i] = self.generator(**self.args)
        return flat.reshape(shape)


def moments_from_sums(mean, moment):
    """Mean, variance and standard deviation of the fidelity over a row's samples AND their gradients with respect to the
    controller, from the two row sums of `backend.mc_fidelity_grad_philox`: `mean` (..., N+2) = (mean F, mean dF/dx) and `moment`
    (..., N+2) = (mean F^2, mean F dF/dx).  NumPy arrays or torch tensors in, the same kind out:

        "fav"      (...,)      mean F                      "grad_fav" (..., N+1)  mean dF/dx
        "var"      (...,)      mean F^2 - fav^2            "grad_var" (..., N+1)  2 (mean F dF/dx - fav grad_fav)
        "std"      (...,)      sqrt(var)                   "grad_std" (..., N+1)  grad_var / (2 std)

    `var` is the ddof = 0 variance - the convention of the `std` metric (np.std) - so that a risk-averse objective
    1 - fav + lambda std and its gradient come from one launch.
    At the rounding floor: `var` is a difference of two numbers of size mean F^2 <= 1, each a sum of K rounded terms, so its
    absolute error is about K eps mean F^2.  Where the computed `var` is at or below 64 * 2^-52 * mean F^2 - the rounding level
    of the subtraction itself - `var`, `std` and `grad_std` are reported as exactly 0 (not a NaN or a quotient of two rounding
    errors); a sigma = 0 row, whose K samples are identical, lands there.  Consequence: below sigma ~ 1e-3 the true variance
    (~ sigma^4 for a controller at a fidelity maximum, ~ sigma^2 elsewhere) is no longer resolved against K eps mean F^2 - form it
    from the per-sample outputs ("fid", "grad") instead."""
    if backend._is_torch(mean):
        import torch as xp
    else:
        xp = np
        mean, moment = np.asarray(mean, dtype=np.float64), np.asarray(moment, dtype=np.float64)
    fav, grad_fav = mean[..., 0], mean[..., 1:]
    m2, mfg = moment[..., 0], moment[..., 1:]
    var = m2 - fav * fav
    floor = var <= (64.0 * 2.0 ** -52) * m2                     # (False in a NaN row: it stays NaN)
    zero = xp.zeros_like(var)
    var = xp.where(floor, zero, var)
    grad_var = 2.0 * (mfg - fav[..., None] * grad_fav)
    std = xp.sqrt(var)
    safe = xp.where(floor, xp.ones_like(std), std)
    grad_std = xp.where(floor[..., None], xp.zeros_like(grad_var), grad_var / (2.0 * safe)[..., None])
    return {"fav": fav, "grad_fav": grad_fav, "var": var, "grad_var": grad_var, "std": std, "grad_std": grad_std}


def readout_jitter_nodes(sigma_t: float, order: int = 8):
    """Gauss-Hermite nodes and weights of a Gaussian readout-time jitter of standard deviation `sigma_t`, as the `tshift` and
    `weights` of `backend.mc_fidelity_times`: with x_j, w_j = numpy.polynomial.hermite.hermgauss(order),
        tshift_j = sqrt(2) sigma_t x_j,    omega_j = w_j / sqrt(pi)        (sum omega = 1).
    With them the kernel's "wsum" is each sample's fidelity averaged over t = T + N(0, sigma_t^2), obtained deterministically
    (exact for fidelities that are polynomials of degree < 2 order in the shift)."""
    if not (float(sigma_t) >= 0.0 and np.isfinite(sigma_t)):
        raise ValueError("sigma_t must be finite and non-negative")
    if not (1 <= int(order) <= backend.MAX_TIMES):
        raise ValueError(f"order must be in 1 .. {backend.MAX_TIMES}")
    x, w = np.polynomial.hermite.hermgauss(int(order))
    return np.sqrt(2.0) * float(sigma_t) * x, w / np.sqrt(np.pi)


# Row lengths at which a GPU tensor goes through `backend.tail_select` (the HIP selection kernel) instead of the torch sort: every
# row length ("Tail selection kernel", has the timing of both routes per shape).
def _tail_select_routed(K: int) -> bool:
    return True


def _tail_plan(fid, alpha):
    alpha = float(alpha)
    if not (0.0 < alpha <= 1.0):
        raise ValueError("alpha must be in (0, 1]")
    if fid.ndim != 2:
        raise ValueError("fid: expected (C, K)")
    K = int(fid.shape[1])
    if K == 0:
        raise ValueError("fid: K must be positive")
    ak = alpha * K
    m = min(K, int(np.ceil(ak)))
    return m, 1.0 / ak, (ak - (m - 1)) / ak


def _tail_weights_torch(fid, alpha: float):
    """`tail_weights` of a torch tensor by torch's stable sort (any device): the route GPU tensors took before the selection
    kernel; kept for CPU tensors, for the timing (scripts/grad_bench.py --select) and as a cross-check."""
    import torch
    m, w_body, w_last = _tail_plan(fid, alpha)
    order = torch.argsort(fid, dim=1, stable=True)[:, :m]
    last = order[:, m - 1:m]
    listed = torch.sort(order, dim=1).values
    weights = torch.full(listed.shape, w_body, dtype=torch.float64, device=fid.device)
    weights[listed == last] = w_last
    bad = torch.isnan(fid).any(dim=1, keepdim=True).expand_as(listed)
    listed = listed.to(torch.int32)
    listed[bad] = -1
    weights[bad] = 0.0
    return listed, weights


def tail_weights(fid, alpha: float):
    """List and weights of the lower tail of each row of `fid` (C, K) for `backend.mc_fidelity_grad_listed`: with them its "sum"
    row is (CVaR_alpha F, d CVaR_alpha / dx) of the row's empirical distribution (Rockafellar - Uryasev; the gradient holds
    almost everywhere: where the tail set does not change).  NumPy array or torch tensor in, the same kind out:

        listed   (C, m) int32     m = ceil(alpha K): the indices of the m smallest values of the row, SORTED ASCENDING (one canonical
                                  summation order); ties go to the lower index
        weights  (C, m) float64   1 / (alpha K), and (alpha K - (m - 1)) / (alpha K) on the m-th smallest: the exact CVaR of the
                                  empirical distribution; every row sums to 1

    alpha in (0, 1]: alpha = 1 gives every index with weight 1 / K (the mean), alpha K < 1 the minimum with weight 1.  A row
    with a NaN in it gives empty slots (-1) with weight 0.
    The NumPy route below is the definition.  A float64 torch tensor on a GPU is selected by the HIP kernel behind
    `backend.tail_select` (same bits, one launch, no sort); a CPU tensor takes torch's stable sort."""
    m, w_body, w_last = _tail_plan(fid, alpha)
    if backend._is_torch(fid):
        if fid.is_cuda and str(fid.dtype) == "torch.float64" and _tail_select_routed(int(fid.shape[1])):
            res = backend.tail_select(fid, alpha, want=("list", "weight"))
            return res["list"], res["weight"]
        return _tail_weights_torch(fid, alpha)
    fid = np.asarray(fid, dtype=np.float64)
    order = np.argsort(fid, axis=1, kind="stable")[:, :m]
    last = order[:, m - 1:m]
    listed = np.sort(order, axis=1)
    weights = np.where(listed == last, w_last, w_body)
    bad = np.isnan(fid).any(axis=1, keepdims=True)
    return np.where(bad, -1, listed).astype(np.int32), np.where(bad, 0.0, weights)


class noise_model_base:
    """Same constructor, attributes and methods as the reference class (noise_model.py:50-115)."""

    def __init__(self, Nspin: int = 5, inspin: int = 0, outspin: int = 2, noise: float = 0.02,
                 topo: str = "chain", rng: noise_function = None, device=None):
        self.Nspin = Nspin
        self.inspin = inspin
        self.outspin = outspin
        self.noise = noise
        self.rng = self.default_gaussian_noise_generator(scale=self.noise) if rng is None else rng
        self.HH = np.zeros((Nspin, Nspin), dtype=np.complex128)
        hop = np.arange(1, Nspin)
        self.HH[hop - 1, hop] = 1
        self.HH[hop, hop - 1] = 1
        if topo == "ring":
            self.HH[Nspin - 1, 0] = 1
            self.HH[0, Nspin - 1] = 1
        self.CC = self.controls()
        self.device = device            # None = torch's current device at call time (one process per GPU)

    def controls(self):
        return [np.diag((np.arange(self.Nspin) == k).astype(np.float64)) for k in range(self.Nspin)]

    def default_gaussian_noise_generator(self, **genargs):
        return noise_function(np.random.normal, **genargs)

    # -- static part of the Hamiltonian as the kernel wants it ------------------------------------
    def _static_terms(self):
        """(h0_diag, h0_offdiag, ring, imag_offdiag) read back from the public `HH` attribute, so that a
        caller who edits `HH` (e.g. adds the XXZ diagonal of qnewton.py:148-150) is honoured."""
        n = self.Nspin
        H = np.asarray(self.HH)
        hop = np.arange(1, n)
        allowed = np.zeros((n, n), dtype=bool)
        allowed[np.arange(n), np.arange(n)] = True
        allowed[hop, hop - 1] = allowed[hop - 1, hop] = True
        ring = bool(n > 2 and (H[n - 1, 0] != 0 or H[0, n - 1] != 0))
        if ring:
            allowed[n - 1, 0] = allowed[0, n - 1] = True
            if not (H[n - 1, 0] == 1 and H[0, n - 1] == 1):
                raise NotImplementedError("ring closure other than J = 1 is not supported by the kernel")
        if (H[~allowed] != 0).any() or not np.allclose(H, H.conj().T, atol=0, rtol=0):
            raise NotImplementedError("HH must be Hermitian nearest-neighbour (chain or ring)")
        diag = H.diagonal().real.copy()
        if (H.diagonal().imag != 0).any():
            raise NotImplementedError("HH must have a real diagonal")
        lower = H[hop, hop - 1]
        return diag, lower.real.copy(), ring, lower.imag.copy()

    # -- sampling ---------------------------------------------------------------------------------
    def draw_samples(self, n_controllers: int, n_draws: int) -> np.ndarray:
        """(C, K, N, 3) draws in the reference's consumption order (controller, draw, site, slot)."""
        raise NotImplementedError

    def perturbation(self) -> np.ndarray:
        raise NotImplementedError

    # -- evaluation -------------------------------------------------------------------------------
    def fidelity_from_draws(self, controllers, draws, kernel: str = "auto", out=None):
        """(C, N+1) controllers x (C, K, N, 3) draws -> (C, K) fidelities on the GPU (`out`: preallocated result)."""
        diag, off, ring, imag = self._static_terms()
        if imag.any():
            if backend._is_torch(draws):
                draws = draws.clone()
                import torch
                draws[..., 1:, 2] += torch.as_tensor(imag, device=draws.device)
            else:
                draws = np.array(draws, dtype=np.float64)
                draws[..., 1:, 2] += imag
        return backend.mc_fidelity(controllers, draws, self.Nspin, self.inspin, self.outspin, h0_diag=diag,
                                   h0_offdiag=off, ring=ring, device=self.device, kernel=kernel, out=out)

    def fidelity_batch(self, controllers, n_draws: int, ham_noisy: bool = True):
        """K noisy evaluations of every controller row; consumes the rng like C*K reference calls."""
        ctrl = np.asarray(controllers, dtype=np.float64).reshape(-1, self.Nspin + 1)
        if ham_noisy:
            draws = self.draw_samples(ctrl.shape[0], n_draws)
        else:
            draws = np.zeros((ctrl.shape[0], n_draws, self.Nspin, 3))
        return self.fidelity_from_draws(ctrl, draws)

    # -- optimiser-side objective over a FIXED set of perturbed Hamiltonians ---------------------------------
    def fixed_perturbation_set(self, size: int, real_only: bool = True) -> np.ndarray:
        """(size, N, 3) draws of a fixed Hamiltonian set, consuming numpy's global stream like the reference's
        `randHset_constructor` (qnewton.py:122-137, after its `np.random.seed(4)`): with `real_only` the
        perturbation is the optimiser's real one (qnewton.py:366-379: per site a diagonal and a coupling draw, no
        imaginary part), otherwise the MC path's three draws per site."""
        sigma = float(self.rng.args.get("scale", self.noise))
        if real_only:
            two = np.random.normal(scale=sigma, size=(size, self.Nspin, 2))
            return np.concatenate([two, np.zeros((size, self.Nspin, 1))], axis=2)
        return np.random.normal(scale=sigma, size=(size, self.Nspin, 3))

    def randHset_constructor(self, train_size: int = 1000, test_size: int = 10000):
        """The optimiser's fixed training / test Hamiltonian sets (qnewton.py:122-137): re-seeds numpy's global stream
        with 4 - as the reference does - and draws `train_size` then `test_size` real perturbations.  Returned as draw
        sets (size, N, 3) in the kernel layout instead of dense matrices."""
        np.random.seed(4)
        return self.fixed_perturbation_set(train_size), self.fixed_perturbation_set(test_size)

    def fidelity_fixed_set(self, controllers, draw_set):
        """(C, R) fidelities of C controllers on ONE set of R perturbations (no replication of the set)."""
        ctrl = np.asarray(controllers, dtype=np.float64).reshape(-1, self.Nspin + 1)
        draw_set = np.ascontiguousarray(draw_set, dtype=np.float64).reshape(1, -1, self.Nspin, 3)
        return self.fidelity_from_draws(ctrl, draw_set)

    def fidelity_ss_av(self, controllers, draw_set, reps=None):
        """Mean fidelity over a fixed set for every controller - the reference's `fidelity_ss_av` (qnewton.py:426-444)
        batched over controllers: `reps` = first Hamiltonians of the set to use (the reference's `test=False` branch
        takes reps = 10 of the training set), None = the whole set (its `test=True` branch)."""
        from . import backend as _be
        draw_set = np.asarray(draw_set, dtype=np.float64).reshape(-1, self.Nspin, 3)
        if reps is not None:
            draw_set = draw_set[: int(reps)]
        fid = self.fidelity_fixed_set(controllers, draw_set)
        return 1.0 - _be.reduce_metrics(fid, q_thresholds=(), overlapped=False)["rim1"][0]

    # -- the objective's analytic gradient (qnewton.py:162-212: what the reference's L-BFGS consumes) --------------------
    def fidelity_grad_from_draws(self, controllers, draws, want=backend.GRAD_OUTPUTS):
        """`backend.mc_fidelity_grad` for this model: (C, N+1) controllers x (C, K, N, 3) or (1, K, N, 3) draws -> dict of
        "fid" (C, K), "grad" (C, K, N+1), "mean" (C, N+2).  Chain topology only."""
        diag, off, ring, imag = self._static_terms()
        if ring:
            raise NotImplementedError("the fidelity gradient is implemented for the chain topology only")
        if imag.any():
            if backend._is_torch(draws):
                draws = draws.clone()
                import torch
                draws[..., 1:, 2] += torch.as_tensor(imag, device=draws.device)
            else:
                draws = np.array(draws, dtype=np.float64)
                draws[..., 1:, 2] += imag
        return backend.mc_fidelity_grad(controllers, draws, self.Nspin, self.inspin, self.outspin, h0_diag=diag,
                                        h0_offdiag=off, device=self.device, want=want)

    def fidelity_ss_av_grad(self, controllers, draw_set, reps=None):
        """`fidelity_ss_av` and its gradient with respect to every controller entry: (fav (C,), grad (C, N+1)), one kernel
        launch for all controllers.  `fav` is the gradient kernel's own row mean: it agrees with `fidelity_ss_av` to
        rounding (another eigensolver route and summation order; both are held to 1e-10), so that value and gradient handed
        to a line search come from the same evaluation."""
        ctrl = np.asarray(controllers, dtype=np.float64).reshape(-1, self.Nspin + 1)
        draw_set = np.asarray(draw_set, dtype=np.float64).reshape(-1, self.Nspin, 3)
        if reps is not None:
            draw_set = draw_set[: int(reps)]
        draws = np.ascontiguousarray(draw_set).reshape(1, -1, self.Nspin, 3)
        mean = self.fidelity_grad_from_draws(ctrl, draws, want=("mean",))["mean"]
        return mean[:, 0].copy(), mean[:, 1:].copy()

    # -- differential sensitivity to the structured noise itself ----------------------------------------------------------
    def fidelity_sens_from_draws(self, controllers, draws, want=backend.SENS_OUTPUTS):
        """`backend.mc_fidelity_sens` for this model: (C, N+1) controllers x (C, K, N, 3) or (1, K, N, 3) draws -> dict of
        "fid" (C, K), "sens" (C, K, N, 3) = dF/d(draw), "mean" (C, 3N+2) = (mean F, mean rho, mean dF/d(draw)).  Chain
        topology only.  rho = sum draw * dF/d(draw) is taken over the DRAWS: the model's static imaginary couplings, which
        the kernel sees as part of its third draw component, are taken out again (rho is linear in the draws, so
        rho = rho_kernel - sum_i imag_i dF/dg2_i exactly, and the same for the row means)."""
        diag, off, ring, imag = self._static_terms()
        if ring:
            raise NotImplementedError("the noise sensitivity is implemented for the chain topology only")
        if imag.any():
            if backend._is_torch(draws):
                draws = draws.clone()
                import torch
                draws[..., 1:, 2] += torch.as_tensor(imag, device=draws.device)
            else:
                draws = np.array(draws, dtype=np.float64)
                draws[..., 1:, 2] += imag
        res = backend.mc_fidelity_sens(controllers, draws, self.Nspin, self.inspin, self.outspin, h0_diag=diag,
                                       h0_offdiag=off, device=self.device, want=want)
        if imag.any() and "mean" in res:
            mean = res["mean"]
            g2 = mean[:, 2:].reshape(mean.shape[0], self.Nspin, 3)[:, 1:, 2]
            if backend._is_torch(mean):
                import torch
                mean[:, 1] -= g2 @ torch.as_tensor(imag, device=mean.device)
            else:
                mean[:, 1] -= g2 @ imag
        return res

    # -- the fidelity on a grid of readout times (early / late readout, timing jitter) ---------------------------------------
    def _times_static(self):
        diag, off, ring, imag = self._static_terms()
        if ring:
            raise NotImplementedError("the readout-time kernels are implemented for the chain topology only")
        return diag, off, imag

    def fidelity_over_times(self, controllers, draws, tscale=None, tshift=None, weights=None, want=("fid",)):
        """`backend.mc_fidelity_times` for this model: (C, N+1) controllers x (C, K, N, 3) or (1, K, N, 3) draws, a grid of M readout
        times t_cj = |T_c tscale_j + tshift_j| -> dict of "fid" (M, C, K), "wsum" (C, K), "min" (C, K) (the entries in `want`) from
        ONE eigen decomposition per sample.  Chain topology only."""
        diag, off, imag = self._times_static()
        if imag.any():
            if backend._is_torch(draws):
                draws = draws.clone()
                import torch
                draws[..., 1:, 2] += torch.as_tensor(imag, device=draws.device)
            else:
                draws = np.array(draws, dtype=np.float64)
                draws[..., 1:, 2] += imag
        return backend.mc_fidelity_times(controllers, draws, self.Nspin, self.inspin, self.outspin, tscale=tscale, tshift=tshift,
                                         weights=weights, want=want, h0_diag=diag, h0_offdiag=off, device=self.device)

    def fidelity_over_times_philox(self, controllers, n_draws: int, seed: int, tscale=None, tshift=None, weights=None,
                                   want=("fid",), sigma=None, offset: int = 0):
        """`fidelity_over_times` over `n_draws` counter-based draws per controller generated INSIDE the kernel
        (`backend.mc_fidelity_times_philox`): no draw tensor, the same bits as `fidelity_over_times(controllers,
        backend.philox_normal((C, K, N, 3), seed, scale=sigma, offset=offset), ...)`; torch tensors out.  `sigma`: None = the
        model's current level; a float; or one value per controller row.  Chain topology with real static couplings only."""
        diag, off, imag = self._times_static()
        if imag.any():
            raise NotImplementedError("draws generated inside the readout-time kernel: real static couplings only (complex ones: "
                                      "fidelity_over_times on a draw tensor)")
        if sigma is None:
            sigma = float(self.rng.args.get("scale", self.noise))
        if not backend._is_torch(controllers):
            controllers = np.asarray(controllers, dtype=np.float64).reshape(-1, self.Nspin + 1)
        return backend.mc_fidelity_times_philox(controllers, int(n_draws), self.Nspin, self.inspin, self.outspin, seed, offset=offset,
                                                sigma=sigma, tscale=tscale, tshift=tshift, weights=weights, want=want, h0_diag=diag,
                                                h0_offdiag=off)

    def fidelity_readout_jitter_philox(self, controllers, n_draws: int, seed: int, sigma_t: float, order: int = 8, sigma=None,
                                       offset: int = 0):
        """(C, K) fidelities, each sample's averaged over a Gaussian jitter of the readout time, t = T + N(0, sigma_t^2), by
        Gauss-Hermite quadrature of `order` nodes (`readout_jitter_nodes`): the "wsum" of ONE `fidelity_over_times_philox` launch.
        NumPy array out.  The structured noise is sampled (`n_draws` counter-based draws per row), the timing jitter integrated."""
        tshift, weights = readout_jitter_nodes(sigma_t, order)
        res = self.fidelity_over_times_philox(controllers, n_draws, seed, tshift=tshift, weights=weights, want=("wsum",),
                                              sigma=sigma, offset=offset)["wsum"]
        return res.cpu().numpy() if backend._is_torch(res) else np.asarray(res)

    def noise_sensitivity(self, controllers, draws):
        """What the samples of ONE sigma level say about the neighbourhood of that level, from one kernel launch:
            "fav"            (C,)       the mean fidelity over the draws (1 - RIM_1),
            "dfav_dlogsigma" (C,)       its slope along the RIM(sigma) curve: for draws = sigma z, d fav / d ln(sigma) at this sigma,
            "direction"      (C, N, 3)  the mean derivative per structured direction, in the draws' layout
                                        ([i][0] site energy i, [i][1] / [i][2] real / imaginary coupling of the sites i - 1, i).
        `draws`: (C, K, N, 3), or one set (K, N, 3) / (1, K, N, 3) shared by every controller.  NumPy arrays out."""
        ctrl = np.asarray(controllers, dtype=np.float64).reshape(-1, self.Nspin + 1)
        if not backend._is_torch(draws):
            draws = np.ascontiguousarray(draws, dtype=np.float64)
        if draws.ndim == 3:
            draws = draws.reshape(1, -1, self.Nspin, 3)
        mean = self.fidelity_sens_from_draws(ctrl, draws, want=("mean",))["mean"]
        if backend._is_torch(mean):
            mean = mean.cpu().numpy()
        return {"fav": mean[:, 0].copy(), "dfav_dlogsigma": mean[:, 1].copy(),
                "direction": mean[:, 2:].reshape(-1, self.Nspin, 3).copy()}

    def noise_sensitivity_philox(self, controllers, n_draws: int, seed: int, sigma=None, offset: int = 0):
        """`noise_sensitivity` over `n_draws` counter-based draws per controller generated INSIDE the kernel
        (`backend.mc_fidelity_sens_philox`): no (C, K, N, 3) tensor, the same dict - and the same bits - as
        `noise_sensitivity(controllers, backend.philox_normal((C, K, N, 3), seed, scale=sigma, offset=offset))`.
        `sigma`: None = the model's current level; a float; or one value per controller row (array or tensor), so that several
        levels of one controller set go through one launch.  Row c, draw k, site i, slot s is stream element
        offset + ((c K + k) N + i) 3 + s.  Chain topology with real static couplings only."""
        diag, off, ring, imag = self._static_terms()
        if ring:
            raise NotImplementedError("the noise sensitivity is implemented for the chain topology only")
        if imag.any():
            raise NotImplementedError("draws generated inside the sensitivity kernel: real static couplings only (complex ones: "
                                      "noise_sensitivity on a draw tensor)")
        if sigma is None:
            sigma = float(self.rng.args.get("scale", self.noise))
        if not backend._is_torch(controllers):
            controllers = np.asarray(controllers, dtype=np.float64).reshape(-1, self.Nspin + 1)
        mean = backend.mc_fidelity_sens_philox(controllers, int(n_draws), self.Nspin, self.inspin, self.outspin, seed, offset=offset,
                                               sigma=sigma, h0_diag=diag, h0_offdiag=off, want=("mean",))["mean"]
        if backend._is_torch(mean):
            mean = mean.cpu().numpy()
        return {"fav": mean[:, 0].copy(), "dfav_dlogsigma": mean[:, 1].copy(),
                "direction": mean[:, 2:].reshape(-1, self.Nspin, 3).copy()}

    def noise_variance_indices_philox(self, controllers, n_draws: int, seed: int, groups="kind", sigma=None, offset: int = 0,
                                      replicates: int = 1):
        """Which noise source is responsible for the spread of the fidelity: the variance-based (first- and total-order) indices
        of groups of noise coordinates by the pick-freeze scheme (`variance_indices` is the definition), from ONE
        `backend.mc_fidelity_pickfreeze_philox` launch over `n_draws` pairs of counter-based draw vectors per controller:
            "fav" (C,) mean fidelity, "var" (C,) its variance over the noise, "first" / "total" (C, G) the indices of every group,
            "groups" (G,) the uint64 masks ("labels": their names).
        `groups`: "direction" (the 3 N - 2 single coordinates), "kind" (site / real / imaginary), "site", or an array of masks over
        the coordinates 3 i + s.  `sigma`: None = the model's current level; a float; or one value per controller row.
        replicates = R >= 2: the rows are tiled R times onto disjoint stream blocks in the same launch - replicate r reads a at
        offset + r C K 3N and b at offset + (R + r) C K 3N -; the values are the means over the replicates and "var_se", "first_se", "total_se"
        their standard errors std(ddof = 1) / sqrt(R).  A sigma = 0 row has var = 0 and NaN indices.  NumPy arrays out.  Chain
        topology with real static couplings, N <= 13 (otherwise NotImplementedError: `variance_indices` on `mc_fidelity` outputs
        of the hybrid tensors serves those)."""
        from . import variance_indices as vi
        diag, off, ring, imag = self._static_terms()
        N = self.Nspin
        if ring:
            raise NotImplementedError("the variance indices are implemented for the chain topology only")
        if imag.any():
            raise NotImplementedError("draws generated inside the pick-freeze kernel: real static couplings only")
        if not backend.pickfreeze_supported(N, ring):
            raise NotImplementedError("the pick-freeze kernel takes chains of N <= 13 spins")
        masks, labels = vi.named_groups(groups, N)
        R, K = int(replicates), int(n_draws)
        if R < 1:
            raise ValueError("replicates must be at least 1")
        if sigma is None:
            sigma = float(self.rng.args.get("scale", self.noise))
        if not backend._is_torch(controllers):
            controllers = np.asarray(controllers, dtype=np.float64).reshape(-1, N + 1)
        C = int(controllers.shape[0])
        per_row = not isinstance(sigma, (int, float)) and np.ndim(sigma) > 0
        if R > 1:                                    # replicate r = rows r C .. (r + 1) C - 1 of ONE launch
            tile = (lambda t: t.repeat(R, *([1] * (t.ndim - 1)))) if backend._is_torch(controllers) else (lambda t: np.tile(t, (R,) + (1,) * (t.ndim - 1)))
            controllers = tile(controllers)
            if per_row:
                sigma = sigma.repeat(R) if backend._is_torch(sigma) else np.tile(np.asarray(sigma, dtype=np.float64), R)
        block = R * C * K * 3 * N                    # a: [offset, offset + block), b: the block behind it
        mean = backend.mc_fidelity_pickfreeze_philox(controllers, K, N, self.inspin, self.outspin, seed, masks, offset=offset,
                                                     offset_b=(int(offset) + block) % 2 ** 64, sigma=sigma, h0_diag=diag,
                                                     h0_offdiag=off, want=("mean",))["mean"]
        mean = mean.cpu().numpy() if backend._is_torch(mean) else np.asarray(mean)
        idx = vi.indices_from_means(mean.reshape(R, C, -1))
        out = {"groups": masks, "labels": labels}
        if R == 1:
            out.update({k: idx[k][0].copy() for k in ("fav", "var", "first", "total")})
            return out
        out["fav"] = idx["fav"].mean(axis=0)
        for k in ("var", "first", "total"):
            out[k], out[k + "_se"] = vi.over_replicates(idx[k])
        return out

    def _moments_of_one_launch(self, launch, controllers, n_draws, seed, sigma, offset, shared):
        """`moments_from_sums` of the "mean" and "moment" rows of one launch of `launch` - `backend.mc_fidelity_grad_philox` or one
        that takes its arguments - with the model's static terms; what `fidelity_moments_philox` and
        `fidelity_jitter_moments_philox` share.  NumPy arrays out."""
        diag, off, ring, imag = self._static_terms()
        if ring:
            raise NotImplementedError("the fidelity gradient is implemented for the chain topology only")
        if imag.any():
            raise NotImplementedError("draws generated inside the gradient kernel: real static couplings only (complex ones: "
                                      "fidelity_grad_from_draws on a draw tensor)")
        if sigma is None:
            sigma = float(self.rng.args.get("scale", self.noise))
        if not backend._is_torch(controllers):
            controllers = np.asarray(controllers, dtype=np.float64).reshape(-1, self.Nspin + 1)
        res = launch(controllers, int(n_draws), self.Nspin, self.inspin, self.outspin, seed, offset=offset, sigma=sigma, shared=shared,
                     h0_diag=diag, h0_offdiag=off, want=("mean", "moment"))
        mean, moment = (v.cpu().numpy() if backend._is_torch(v) else np.asarray(v) for v in (res["mean"], res["moment"]))
        return {k: v.copy() for k, v in moments_from_sums(mean, moment).items()}

    def fidelity_moments_philox(self, controllers, n_draws: int, seed: int, sigma=None, offset: int = 0, shared: bool = False):
        """Mean, variance and standard deviation of the fidelity over `n_draws` counter-based draws per controller generated
        INSIDE the gradient kernel, with their gradients with respect to the controller: `moments_from_sums` of the "mean" and
        "moment" rows of ONE `backend.mc_fidelity_grad_philox` launch (no per-sample output, no draw tensor).  NumPy arrays out.
        `sigma`: None = the model's current level; a float; or one value per controller row.  shared=False: row c, draw k, site
        i, slot s is stream element offset + ((c K + k) N + i) 3 + s; shared=True (common random numbers: the same draws for
        every controller, the `fidelity_ss_av` kind of objective): offset + (k N + i) 3 + s.  Chain topology with real static
        couplings only."""
        return self._moments_of_one_launch(backend.mc_fidelity_grad_philox, controllers, n_draws, seed, sigma, offset, shared)

    def fidelity_rqmc(self, controllers, replicates: int = 16, points: int = 1024, seed: int = 0, sigma=None, skip: int = 0,
                      shared: bool = True):
        """Randomised quasi-Monte Carlo estimate of the mean fidelity of every controller row, with its standard error: `replicates`
        independently scrambled Sobol point sets (`sobol.scramble(3 N, replicates, seed)`: linear matrix scrambling + digital shift)
        of `points` points each -> {"mean": (C,), "se": (C,), "replicate_means": (C, R)}, se = std of the R replicate means
        (ddof = 1) / sqrt(R).  ONE fidelity launch - `backend.mc_fidelity_sobol` for chains of N <= 13 spins, the generator
        `backend.sobol_normal` + the tensor kernel otherwise - plus `backend.reduce_metrics` on the (C R, P) view of fid (C, R P).
        `sigma`: None = the model's current level; a float; or one value per controller row.  shared=True: every row reads the
        same shifts (common random numbers); False: a shift row per controller.  NumPy arrays out."""
        rep = self.fidelity_rqmc_replicates(controllers, replicates, points, seed, sigma=sigma, skip=skip, shared=shared)
        means = 1.0 - rep["rim1"]
        return {"mean": means.mean(axis=1), "se": means.std(axis=1, ddof=1) / np.sqrt(means.shape[1]), "replicate_means": means}

    def fidelity_rqmc_replicates(self, controllers, replicates: int, points: int, seed: int, sigma=None, skip: int = 0,
                                 shared: bool = True):
        """The launch behind `fidelity_rqmc`: per controller row and scrambled replicate the centre metrics of
        `backend.reduce_metrics` over the replicate's `points` fidelities -> {"rim1", "std", "min"}, each a (C, R) NumPy array."""
        from . import sobol
        diag, off, ring, imag = self._static_terms()
        R, P, N = int(replicates), int(points), self.Nspin
        if R < 2:
            raise ValueError("replicates must be at least 2 (the standard error is taken over them)")
        if sigma is None:
            sigma = float(self.rng.args.get("scale", self.noise))
        if not backend._is_torch(controllers):
            controllers = np.asarray(controllers, dtype=np.float64).reshape(-1, N + 1)
        C = int(controllers.shape[0])
        dirnum, shift = sobol.scramble(3 * N, R, seed, C=None if shared else C)
        if backend.sobol_fused_supported(N, ring) and not imag.any():
            fid = backend.mc_fidelity_sobol(controllers, R * P, N, self.inspin, self.outspin, dirnum, shift, P, skip=skip, sigma=sigma,
                                            h0_diag=diag, h0_offdiag=off)
        else:
            draws = backend.sobol_normal(dirnum, shift, P, R * P, skip=skip, sigma=sigma, C=C, device=self.device, as_torch=True)
            fid = self.fidelity_from_draws(controllers if backend._is_torch(controllers) else np.ascontiguousarray(controllers),
                                           draws.view(C, R * P, N, 3))
        red = backend.reduce_metrics(fid.reshape(C * R, P), q_thresholds=(), overlapped=False)
        host = lambda v: v.cpu().numpy() if backend._is_torch(v) else np.asarray(v)
        return {k: host(red[k])[0].reshape(C, R) for k in ("rim1", "std", "min")}

    def fidelity_jitter_moments_philox(self, controllers, n_draws: int, seed: int, sigma_t: float, order: int = 8, sigma=None,
                                       offset: int = 0, shared: bool = False):
        """`fidelity_moments_philox` of the fidelity AVERAGED OVER A GAUSSIAN READOUT-TIME JITTER of standard deviation `sigma_t`:
        with W = E_delta F(T + delta) by the `order`-point Gauss-Hermite rule of `readout_jitter_nodes`, the mean, variance and
        standard deviation of W over the draws and their gradients with respect to the controller (the time entry included) -
        `moments_from_sums` of the "mean" and "moment" rows of ONE `backend.mc_fidelity_grad_times_philox` launch, one eigen
        decomposition per sample for the whole rule.  The same dict as `fidelity_moments_philox`; the other arguments as there."""
        tshift, weights = readout_jitter_nodes(sigma_t, order)

        def launch(*args, **kw):
            return backend.mc_fidelity_grad_times_philox(*args, tshift=tshift, weights=weights, **kw)
        return self._moments_of_one_launch(launch, controllers, n_draws, seed, sigma, offset, shared)

    @staticmethod
    def _jitter_grid(jitter):
        """`optimize_controllers`' `jitter` as the grid keywords of `backend.mc_fidelity_grad_times_philox`: sigma_t, (sigma_t,
        order) - the Gauss-Hermite rule of `readout_jitter_nodes` - or dict(tscale=, tshift=, weights=) taken as it is"""
        if isinstance(jitter, dict):
            unknown = set(jitter) - {"tscale", "tshift", "weights"}
            if unknown or jitter.get("weights") is None:
                raise ValueError("jitter: dict(tscale=, tshift=, weights=) with weights")
            tscale, tshift, weights = backend._times_grid(jitter.get("tscale"), jitter.get("tshift"), jitter["weights"])
            return {"tscale": tscale, "tshift": tshift, "weights": weights}      # (host vectors: nothing is converted per evaluation)
        sigma_t, order = (jitter if isinstance(jitter, (tuple, list)) else (jitter, 8))
        tshift, weights = readout_jitter_nodes(float(sigma_t), int(order))
        return {"tscale": None, "tshift": tshift, "weights": weights}

    def _cvar_device(self, ctrl, K: int, seed: int, alpha: float, sigma, offset: int, shared: bool, diag, off):
        """The device-resident part of `fidelity_cvar_philox`: ctrl (C, N+1) float64 CUDA tensor, `sigma` a float or a (C,) tensor
        on its device -> (sum (C, N+2) = (CVaR, d CVaR / dx), var (C,)) as tensors on the current stream, nothing synchronised:
        the fidelity launch, the tail selection and the listed-sample gradient launch."""
        import torch
        N = self.Nspin
        rows = np.ndim(sigma) > 0
        if not shared:
            fid = backend.mc_fidelity_philox(ctrl, K, N, self.inspin, self.outspin, seed, offset=offset, sigma=sigma, h0_diag=diag,
                                             h0_offdiag=off)
        elif not rows:
            with torch.cuda.device(ctrl.device):
                draws = backend.philox_normal((1, K, N, 3), seed, scale=float(sigma), offset=offset, as_torch=True)
            fid = backend.mc_fidelity(ctrl, draws, N, self.inspin, self.outspin, h0_diag=diag, h0_offdiag=off)
        else:                                      # (one draw set, one scale per row: no fidelity-only kernel takes that)
            fid = backend.mc_fidelity_grad_philox(ctrl, K, N, self.inspin, self.outspin, seed, offset=offset, sigma=sigma, shared=True,
                                                  h0_diag=diag, h0_offdiag=off, want=("fid",))["fid"]
        if _tail_select_routed(K):                 # list, weights and value at risk from ONE selection launch
            sel = backend.tail_select(fid, alpha)
            listed, weights, var = sel["list"], sel["weight"], sel["var"]
        else:
            listed, weights = _tail_weights_torch(fid, alpha)
            var = torch.gather(fid, 1, listed.clamp(min=0).long()).max(dim=1).values   # (a NaN row gathers NaN)
        res = backend.mc_fidelity_grad_listed(ctrl, K, listed, weights, nspin=N, inspin=self.inspin, outspin=self.outspin, seed=seed,
                                              offset=offset, sigma=sigma, shared=shared, h0_diag=diag, h0_offdiag=off, want=("sum",))
        return res["sum"], var

    def fidelity_cvar_philox(self, controllers, n_draws: int, seed: int, alpha: float, sigma=None, offset: int = 0,
                             shared: bool = False):
        """CVaR_alpha of the fidelity - the mean of the worst alpha K of `n_draws` counter-based draws per controller - with its
        gradient with respect to the controller: {"cvar" (C,), "grad_cvar" (C, N+1), "var" (C,)}, NumPy arrays.  Three launches,
        nothing per sample leaves the device: the fidelities of all K draws (`backend.mc_fidelity_philox`, the mixed-precision
        kernel), ONE selection launch (`backend.tail_select`: list, weights, value at risk), and ONE
        `backend.mc_fidelity_grad_listed` launch over the selected ceil(alpha K) draws with want=("sum",).  "cvar" is that launch's own weighted sum, so value and gradient come from one evaluation;
        "var" - the value at risk - is the largest selected fidelity.  The gradient is that of the empirical CVaR where the tail
        set is locally constant (almost everywhere).  A NaN row gives NaN.  alpha = 1: the mean and its gradient.
        `sigma`, `offset`, `shared` and the restrictions (chain topology, real static couplings): as `fidelity_moments_philox`."""
        diag, off, ring, imag = self._static_terms()
        if ring:
            raise NotImplementedError("the fidelity gradient is implemented for the chain topology only")
        if imag.any():
            raise NotImplementedError("draws generated inside the gradient kernel: real static couplings only (complex ones: "
                                      "fidelity_grad_from_draws on a draw tensor)")
        if not (0.0 < float(alpha) <= 1.0):
            raise ValueError("alpha must be in (0, 1]")
        if int(n_draws) < 1:
            raise ValueError("n_draws must be positive")
        if sigma is None:
            sigma = float(self.rng.args.get("scale", self.noise))
        if not backend._is_torch(controllers):
            controllers = np.asarray(controllers, dtype=np.float64).reshape(-1, self.Nspin + 1)
        import torch
        ctrl = (controllers if backend._is_torch(controllers) else torch.from_numpy(controllers).to(backend.compute_device()))
        ctrl = ctrl.to(dtype=torch.float64).contiguous()
        if np.ndim(sigma) > 0:
            sigma = (sigma if backend._is_torch(sigma) else torch.from_numpy(np.ascontiguousarray(sigma, dtype=np.float64)))
            sigma = sigma.to(device=ctrl.device, dtype=torch.float64)
        total, var = self._cvar_device(ctrl, int(n_draws), seed, alpha, sigma, offset, shared, diag, off)
        total = total.cpu().numpy()
        nan = np.isnan(ctrl.cpu().numpy()).any(axis=1)
        var = var.cpu().numpy().copy()
        var[nan] = np.nan
        return {"cvar": total[:, 0].copy(), "grad_cvar": total[:, 1:].copy(), "var": var}

    def optimize_controllers(self, controllers, n_draws: int, seed: int, objective="mean", sigma=None, offset: int = 0,
                             shared: bool = True, mask=None, max_evals: int = 60, poll: int = 8, bounds=None, jitter=None,
                             **lbfgs_params):
        """Robust re-optimisation of ALL controller rows at once by the batched L-BFGS state machine on the device
        (`backend.lbfgs_init` / `lbfgs_advance`; the definition is `lbfgs.py`): per evaluation ONE gradient launch over the rows'
        trial points and one advance launch, everything device-resident on the current stream.  Objective, over `n_draws`
        counter-based draws per row generated inside the kernels:

            "mean"             1 - mean F                        `mc_fidelity_grad_philox`, want = ("mean",)
            ("std", lam)       1 - mean F + lam std F            ... want = ("mean", "moment")
            ("cvar", alpha)    1 - CVaR_alpha F                  the three launches of `fidelity_cvar_philox`

        `jitter` (None = off: exactly the launches above): sigma_t, (sigma_t, order) or dict(tscale=, tshift=, weights=) - F is
        replaced by W = E_delta F(T + delta), its average over a Gaussian readout-time jitter of standard deviation sigma_t (the
        Gauss-Hermite rule of `readout_jitter_nodes`, order 8 by default) or over the given grid, and the "mean" and ("std", lam)
        objectives are evaluated by ONE `mc_fidelity_grad_times_philox` launch per evaluation (one eigen decomposition per sample
        for the whole grid; the grid goes to the device once).  ("cvar", alpha) with `jitter`: NotImplementedError.

        shared=True (common random numbers, the default): every row and every evaluation sees the same draws, so the objective is
        a deterministic function of the controller - what a line search needs.  `mask` (C, N+1) of 0 / 1 or None: a masked entry
        never moves (mask[:, N] = 0 fixes the time T).  `bounds` = (lo, hi), each a scalar, (N+1,) or (C, N+1), NumPy or torch,
        -inf / +inf for a side without a bound: the boxed machine - the start rows are projected into the box, every trial point
        and the returned `x` lie inside it, and status 1 is the projected-gradient test.  `lbfgs_params`: m (5), c1 (1e-4),
        gtol (1e-6), ftol (0 = off), maxiter (100), maxback (20).  At most `max_evals` evaluations; every `poll` evaluations the
        status column is copied to the host and the loop stops when no row is running - the only synchronisation.
        Returns NumPy arrays {"x" (C, N+1), "f" (C,), "grad" (C, N+1), "status" (C,), "iters" (C,), "evals" (C,)}: the best
        accepted point of every row, its objective value and gradient; status 0 = still running after `max_evals`, 1 gtol, 2
        ftol, 3 maxiter, 4 line search failed, 5 not finite / NaN row.  Chain topology with real static couplings, N <= 12, one
        GPU."""
        diag, off, ring, imag = self._static_terms()
        if ring:
            raise NotImplementedError("the fidelity gradient is implemented for the chain topology only")
        if imag.any():
            raise NotImplementedError("draws generated inside the gradient kernel: real static couplings only")
        if objective == "mean":
            kind, par = "one_minus", 0.0
        elif isinstance(objective, (tuple, list)) and len(objective) == 2 and objective[0] in ("std", "cvar"):
            kind, par = ("one_minus_plus_std" if objective[0] == "std" else "cvar"), float(objective[1])
            if kind == "cvar" and not (0.0 < par <= 1.0):
                raise ValueError("alpha must be in (0, 1]")
        else:
            raise ValueError('objective: "mean", ("std", lam) or ("cvar", alpha)')
        grid = None
        if jitter is not None:
            if kind == "cvar":
                raise NotImplementedError("the CVaR objective under readout jitter (the listed-sample kernel has no time grid)")
            grid = self._jitter_grid(jitter)
        K, N = int(n_draws), self.Nspin
        if K < 1 or int(max_evals) < 1 or int(poll) < 1:
            raise ValueError("n_draws, max_evals and poll must be positive")
        m = int(lbfgs_params.pop("m", 5))
        unknown = set(lbfgs_params) - set(backend.LBFGS_DEFAULTS)
        if bounds is not None and not (isinstance(bounds, (tuple, list)) and len(bounds) == 2):
            unknown.add("bounds")                                     # (only a pair (lo, hi) is the bounds keyword)
        if unknown:
            raise ValueError(f"unknown L-BFGS parameters {sorted(unknown)} (bounds is a pair (lo, hi))")
        if sigma is None:
            sigma = float(self.rng.args.get("scale", self.noise))
        import torch
        if not backend._is_torch(controllers):
            controllers = torch.from_numpy(np.asarray(controllers, dtype=np.float64).reshape(-1, N + 1)).to(backend.compute_device())
        x0 = controllers.to(dtype=torch.float64).contiguous()
        if tuple(x0.shape[1:]) != (N + 1,):
            raise ValueError(f"controllers: expected (C, {N + 1})")
        dev = x0.device
        if np.ndim(sigma) > 0:
            sigma = (sigma if backend._is_torch(sigma) else torch.from_numpy(np.ascontiguousarray(sigma, dtype=np.float64)))
            sigma = sigma.to(device=dev, dtype=torch.float64)
        if mask is not None:
            mask = (mask if backend._is_torch(mask) else torch.from_numpy(np.array(np.broadcast_to(np.asarray(mask, dtype=np.float64),
                                                                                                 tuple(x0.shape)))))
            mask = mask.to(device=dev, dtype=torch.float64).contiguous()
        box = {}
        if bounds is not None:                                        # on the device once, the same two tensors at every call
            as_rows = lambda b: (b if backend._is_torch(b) else torch.from_numpy(np.array(b, dtype=np.float64))).to(
                device=dev, dtype=torch.float64).expand(tuple(x0.shape)).contiguous()
            box = {"bounds": (as_rows(bounds[0]), as_rows(bounds[1]))}
        geo = dict(h0_diag=diag, h0_offdiag=off)
        state, trial = backend.lbfgs_init(x0, mask, m=m, **box)
        status = state[lbfgs.field_offsets(N + 1, m)["status"]]
        for ev in range(1, int(max_evals) + 1):
            row_b = None
            if kind == "cvar":
                row_a, _ = self._cvar_device(trial, K, seed, par, sigma, offset, shared, diag, off)
            else:
                want = ("mean", "moment") if kind == "one_minus_plus_std" else ("mean",)
                if grid is None:
                    res = backend.mc_fidelity_grad_philox(trial, K, N, self.inspin, self.outspin, seed, offset=offset, sigma=sigma,
                                                          shared=shared, want=want, **geo)
                else:                                                 # (the grid's device copy is made at the first evaluation)
                    res = backend.mc_fidelity_grad_times_philox(trial, K, N, self.inspin, self.outspin, seed, offset=offset,
                                                                sigma=sigma, shared=shared, want=want, **grid, **geo)
                row_a, row_b = res["mean"], res.get("moment")
            backend.lbfgs_advance(state, trial, row_a, row_b, m=m, kind="one_minus" if kind == "cvar" else kind, lam=par,
                                  **box, **lbfgs_params)
            if ev % int(poll) == 0 and ev < int(max_evals) and not bool((status == 0.0).any().item()):
                break
        res = backend.lbfgs_result(state, trial, m=m)
        return {k: v.cpu().numpy() for k, v in res.items()}

    def nominal_sensitivity(self, controllers):
        """(C, N, 3): dF/d(perturbation) of the unperturbed system per structured direction - the differential sensitivity at
        sigma = 0.  The imaginary-coupling column is exactly 0 when the static couplings are real (F is even in it)."""
        ctrl = np.asarray(controllers, dtype=np.float64).reshape(-1, self.Nspin + 1)
        zero = np.zeros((1, 1, self.Nspin, 3))
        return self.fidelity_sens_from_draws(ctrl, zero, want=("sens",))["sens"][:, 0].copy()

    # -- the scalar API -----------------------------------------------------------------------------------------------
    # Reference-style callers loop `for b in range(K): f += nm.evaluate_noisy_fidelity(cont, ham_noisy=True)`
    # (gen_fig_8_arim_fcall_scaling.py:121-132).  One GPU launch + sync per sample costs what the reference's CPU
    # evaluation costs, and there is no CPU path to fall back to.  So a call LOOKS AHEAD: after drawing its own 3N
    # perturbations from numpy's stream - exactly what the reference does at this point - it also draws those of the
    # next B - 1 samples, evaluates all B in one launch, and puts the generator back to where it was after ITS sample.
    # A following call again draws its 3N values from the live stream and compares them with the ones the block was
    # computed from: equal draws (and same controller, sigma, Hamiltonian) => the stored fidelity IS this sample's
    # fidelity; anything else (somebody drew from numpy in between, `rng(scale=...)` burned a draw, another controller)
    # => the values just drawn are still this sample's draws, a new block starts from them.  `np.random`'s state is the
    # reference's at every call boundary, bit for bit, without ever being inspected.  B grows 8 -> 1024 on hits.
    _LOOKAHEAD_MAX = 1024

    def _lookahead_usable(self) -> bool:
        return type(self).draw_samples is structured_perturbation.draw_samples and backend.legacy_stream_usable(self.rng)

    def _lookahead_eval(self, x: np.ndarray) -> float:
        sigma = float(self.rng.args.get("scale", self.noise))
        shape = (self.Nspin, 3)
        mine = np.random.normal(scale=sigma, size=shape)           # this sample's draws: consumed like the reference does
        la = self.__dict__.get("_la")
        sig = (x.tobytes(), sigma, np.asarray(self.HH).tobytes(), self.inspin, self.outspin)   # HH is public and mutable
        if la is not None and la["sig"] == sig and la["i"] < len(la["fid"]) and np.array_equal(mine, la["draws"][la["i"]]):
            la["i"] += 1
            return float(la["fid"][la["i"] - 1])
        block = 8 if la is None or la["sig"] != sig else min(self._LOOKAHEAD_MAX, 2 * len(la["fid"]))
        here = np.random.get_state()
        draws = np.empty((block,) + shape)
        draws[0] = mine
        draws[1:] = np.random.normal(scale=sigma, size=(block - 1,) + shape)       # the following samples' draws
        np.random.set_state(here)                                  # ... which the reference has not consumed yet
        fid = np.asarray(self.fidelity_from_draws(x, draws[None]))[0]
        self._la = {"sig": sig, "fid": fid, "draws": draws, "i": 1}
        return float(fid[0])

    def evaluate_noisy_fidelity(self, x, ham_noisy: bool = False):
        """One sample, reference signature (noise_model.py:98-109)."""
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(1, -1)[:, : self.Nspin + 1])
        if ham_noisy and self._lookahead_usable():
            return self._lookahead_eval(x)
        return float(self.fidelity_batch(x, 1, ham_noisy)[0, 0])


class structured_perturbation(noise_model_base):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)

    def draw_samples(self, n_controllers: int, n_draws: int) -> np.ndarray:
        return self.rng.draw_block((n_controllers, n_draws, self.Nspin, 3))

    def perturbation(self) -> np.ndarray:
        """Dense matrix form of ONE sample (API parity with noise_model.py:122-147; the hot path never
        materialises it).  Consumes 3N draws."""
        g = self.draw_samples(1, 1)[0, 0]
        n = self.Nspin
        z = np.zeros((n, n), dtype=np.complex128)
        z[np.arange(n), np.arange(n)] = g[:, 0]
        lo = np.arange(1, n)
        z[lo, lo - 1] = g[1:, 1] + 1j * g[1:, 2]
        z[lo - 1, lo] = g[1:, 1] - 1j * g[1:, 2]
        return z


class directional_perturbation(noise_model_base):
    """One random element pair of the Hamiltonian perturbed per sample (noise_model.py:150-201).

    Per sample the reference consumes ``np.random.randint(0, len(directions))`` and then ``rng(size=2)`` (which
    also makes ``size=2`` sticky on the generator, as there).  For a bond direction the perturbation is Hermitian;
    for a diagonal direction (i, i) the second assignment ``z[i,i] = a - ib`` overwrites the first, so the
    Hamiltonian gets a complex diagonal entry and is NOT Hermitian - evaluated by the dense Pade-expm kernel
    (`backend.mc_fidelity_nonhermitian`), like every sample of this model.
    """

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        n = self.Nspin
        self.directions = [(0, 0), (n - 1, n - 1)]
        for d in range(1, n - 1):
            for o in (-1, 0, 1):
                self.directions.append((d, d + o))
        self.directions += [(0, 1), (1, 0), (n - 2, n - 1), (n - 1, n - 2)]

    def _draw_one(self):
        idx = np.random.randint(low=0, high=len(self.directions))
        nval = self.rng(size=2)
        return self.directions[idx], float(nval[0]), float(nval[1])

    def perturbation(self) -> np.ndarray:
        (p, q), a, b = self._draw_one()
        z = np.zeros((self.Nspin, self.Nspin), dtype=np.complex128)
        z[p, q] = a + 1j * b
        z[q, p] = a - 1j * b
        return z

    def _draw_indices(self, n: int):
        """(direction index [n], (a, b) [n, 2]) of n samples, consuming numpy's global stream sample by sample exactly
        like n calls of the reference's `perturbation()`: `np.random.randint(0, len(directions))`, then `rng(size=2)`.
        With the default generator the whole sequence is produced by the library's host-side emulation of the legacy
        stream (`rc_directional_draws_legacy`: bit-identical indices, normals and generator state, ~100x the Python
        loop); any other generator takes the sample-by-sample loop."""
        import ctypes
        from . import _lib
        rng = self.rng
        if not self._plain_legacy() or n == 0:
            idx = np.empty(n, dtype=np.int32)
            ab = np.empty((n, 2))
            for i in range(n):
                idx[i] = np.random.randint(low=0, high=len(self.directions))
                ab[i] = self.rng(size=2)
            return idx, ab
        lib = _lib.load()
        name, key, pos, has_gauss, cached = np.random.get_state()
        st = _lib.Mt19937State()
        ctypes.memmove(st.key, np.ascontiguousarray(key, dtype=np.uint32).ctypes.data, 624 * 4)
        st.pos, st.has_gauss, st.gauss = int(pos), int(has_gauss), float(cached)
        idx = np.empty(n, dtype=np.int32)
        ab = np.empty((n, 2))
        sigma = float(rng.args.get("scale", self.noise))
        rc = lib.rc_directional_draws_legacy(ctypes.byref(st), n, len(self.directions), sigma,
                                             ctypes.c_void_p(idx.ctypes.data), ctypes.c_void_p(ab.ctypes.data))
        if rc != 0:
            raise ValueError("rc_directional_draws_legacy failed")
        np.random.set_state(("MT19937", np.frombuffer(st.key, dtype=np.uint32).copy(), int(st.pos), int(st.has_gauss),
                             float(st.gauss)))
        rng.args["size"] = 2                          # `rng(size=2)` is sticky on the generator, as in the reference
        return idx, ab

    def draw_samples(self, n_controllers: int, n_draws: int):
        """(draws (C, K, N, 3), diag_imag (C, K, N)) in the kernel layout, consuming the RNG sample by sample in
        (controller, draw) order exactly like C*K calls of the reference's `perturbation()`."""
        idx, ab = self._draw_indices(n_controllers * n_draws)
        return self._layout(idx, ab, n_controllers, n_draws)

    def _layout(self, idx, ab, n_controllers: int, n_draws: int):
        """The dense kernel layout (draws (C, K, N, 3), diag_imag (C, K, N)) of samples given as (direction index, a, b)."""
        n = self.Nspin
        total = n_controllers * n_draws
        dirs = np.asarray(self.directions, dtype=np.int64)            # (3N - 2, 2)
        p, q = dirs[idx, 0], dirs[idx, 1]
        a, b = ab[:, 0], ab[:, 1]
        draws = np.zeros((total, n, 3))
        imag = np.zeros((total, n))
        s = np.arange(total)
        diag = p == q
        draws[s[diag], p[diag], 0] = a[diag]          # z[p,p] = a + ib, then overwritten by a - ib (noise_model.py:196-199)
        imag[s[diag], p[diag]] = -b[diag]
        low = p == q + 1                              # z[p][p-1] = a + ib: the lower element of bond p
        draws[s[low], p[low], 1], draws[s[low], p[low], 2] = a[low], b[low]
        up = p == q - 1                               # z[p][p+1] = a + ib -> lower element z[q][p] = a - ib
        draws[s[up], q[up], 1], draws[s[up], q[up], 2] = a[up], -b[up]
        return draws.reshape(n_controllers, n_draws, n, 3), imag.reshape(n_controllers, n_draws, n)

    # The scalar API of this model looks ahead like the structured model's (noise_model_base._lookahead_eval): a call draws its
    # own sample from numpy's stream exactly as the reference does (randint, then rng(size=2)), plus - through the bit-identical
    # host emulation of that consumption - the next B - 1 samples, evaluates all B at once and puts the generator back; the
    # following calls compare what they draw with what the block was computed from.  (Round 3: one launch + sync per sample.)
    def _lookahead_usable(self) -> bool:
        return self._plain_legacy()

    def _lookahead_eval(self, x: np.ndarray) -> float:
        sigma = float(self.rng.args.get("scale", self.noise))
        idx0 = int(np.random.randint(low=0, high=len(self.directions)))      # this sample, consumed like the reference does
        ab0 = np.asarray(self.rng(size=2), dtype=np.float64)
        la = self.__dict__.get("_la")
        sig = (x.tobytes(), sigma, np.asarray(self.HH).tobytes(), self.inspin, self.outspin)
        if la is not None and la["sig"] == sig and la["i"] < len(la["fid"]) and idx0 == la["idx"][la["i"]] \
                and np.array_equal(ab0, la["ab"][la["i"]]):
            la["i"] += 1
            return float(la["fid"][la["i"] - 1])
        block = 8 if la is None or la["sig"] != sig else min(self._LOOKAHEAD_MAX, 2 * len(la["fid"]))
        here = np.random.get_state()
        idx_n, ab_n = self._draw_indices(block - 1)                # the following samples' draws ...
        np.random.set_state(here)                                  # ... which the reference has not consumed yet
        idx = np.concatenate([[idx0], idx_n]).astype(np.int32)
        ab = np.concatenate([ab0[None, :], ab_n], axis=0)
        draws_t, imag = self._layout(idx, ab, 1, block)
        fid = np.asarray(self._fidelity_from_layout(x, draws_t, imag))[0]
        self._la = {"sig": sig, "fid": fid, "idx": idx, "ab": ab, "i": 1}
        return float(fid[0])

    def _plain_legacy(self) -> bool:
        rng = self.rng
        return (getattr(rng, "generator", None) is np.random.normal and set(rng.args) <= {"scale", "loc", "size"}
                and float(rng.args.get("loc", 0.0)) == 0.0 and rng.args.get("size", 2) == 2)

    def fidelity_batch(self, controllers, n_draws: int, ham_noisy: bool = True, draws: str = "auto"):
        """(C, K) fidelities.  A bond direction is a Hermitian sample of the ordinary draw layout: ALL samples first go
        through the fast chain / ring kernels (imaginary diagonal ignored); the diagonal directions - a complex diagonal
        entry, non-Hermitian - are then recomputed by the dense Pade-expm kernel on a compacted list and put in place.

        draws="device" (what "auto" picks for the default generator on a GPU): the RNG consumption itself runs on the
        GPU (`backend.directional_draws_device`), 20 bytes per sample are all that exists of a sample before the layout
        is expanded ON the device, and only the (C, K) result crosses PCIe.  draws="host": the bit-identical host
        emulation / the sample-by-sample loop for custom generators, layout built with NumPy (round 2)."""
        ctrl = np.asarray(controllers, dtype=np.float64).reshape(-1, self.Nspin + 1)
        if draws not in ("auto", "device", "host"):
            raise ValueError("draws must be 'auto', 'device' or 'host'")
        total = ctrl.shape[0] * n_draws
        # "auto": the device pipeline pays a few launches and two synchronisations - worth it from a few thousand samples
        # on; the scalar API (one sample per call) keeps the host emulation
        # ("auto" also asks that the device-continued normals ARE NumPy's on this host - backend.legacy_device_exact)
        if ham_noisy and self._plain_legacy() and (draws == "device" and total > 0 or
                                                   draws == "auto" and total >= 2048 and backend.legacy_device_exact()):
            return self._fidelity_batch_device(ctrl, n_draws)
        if draws == "device" and ham_noisy:
            raise ValueError("draws='device' needs the default generator (np.random.normal)")
        if ham_noisy:
            draws_t, imag = self.draw_samples(ctrl.shape[0], n_draws)
        else:
            draws_t, imag = np.zeros((ctrl.shape[0], n_draws, self.Nspin, 3)), None
        return self._fidelity_from_layout(ctrl, draws_t, imag)

    def _fidelity_from_layout(self, ctrl, draws_t, imag):
        """(C, K) fidelities of samples in the dense layout: everything through the fast Hermitian kernels, the samples with
        an imaginary diagonal entry (diagonal directions) recomputed by the non-Hermitian entry and put in place."""
        diag, off, ring, imag_off = self._static_terms()
        if imag_off.any():
            draws_t[..., 1:, 2] += imag_off
        fid = np.asarray(backend.mc_fidelity(ctrl, draws_t, self.Nspin, self.inspin, self.outspin, h0_diag=diag, h0_offdiag=off,
                                             ring=ring, device=self.device))
        if imag is not None:
            cs, ks = np.nonzero(imag.any(axis=2))                  # the non-Hermitian samples
            if cs.size:
                sub = backend.mc_fidelity_nonhermitian(ctrl[cs], draws_t[cs, ks][:, None], imag[cs, ks][:, None], self.Nspin,
                                                       self.inspin, self.outspin, h0_diag=diag, h0_offdiag=off, ring=ring,
                                                       device=self.device)
                fid[cs, ks] = np.asarray(sub)[:, 0]
        return fid

    def _fidelity_batch_device(self, ctrl: np.ndarray, n_draws: int) -> np.ndarray:
        """The device-resident pipeline of `fidelity_batch`: (index, a, b) per sample from the GPU-side continuation of
        numpy's stream, the (C, K, N, 3) layout scattered from them on the device, the fast kernels on everything, the
        Pade-expm kernel on the compacted diagonal-direction samples."""
        import torch
        n, C, K = self.Nspin, ctrl.shape[0], n_draws
        total = C * K
        sigma = float(self.rng.args.get("scale", self.noise))
        idx, ab = backend.directional_draws_device(total, len(self.directions), sigma, device=self.device)
        self.rng.args["size"] = 2                     # `rng(size=2)` is sticky on the generator, as in the reference
        dev = idx.device
        diag, off, ring, imag_off = self._static_terms()
        if not ring and n <= 12 and not imag_off.any():
            # round 4: ONE library call from the 20 bytes per sample to the fidelities - class partition, real tridiagonal
            # routes for the bond directions, complex symmetric QL for the diagonal ones (k_directional.inc.h); nothing of the
            # (C, K, N, 3) layout is ever built
            fid = backend.mc_fidelity_directional(torch.as_tensor(ctrl, device=dev), idx, ab, n, self.inspin, self.outspin, K,
                                                  h0_diag=diag, h0_offdiag=off)
            return self._to_host(fid)
        # rings, N > 12, complex static couplings: the dense layout, scattered on the device
        dirs = torch.as_tensor(np.asarray(self.directions, dtype=np.int64), device=dev)       # (3N - 2, 2)
        pq = dirs[idx.long()]
        p, q = pq[:, 0], pq[:, 1]
        a, b = ab[:, 0], ab[:, 1]
        draws = torch.zeros((total, n, 3), dtype=torch.float64, device=dev)
        s = torch.arange(total, device=dev)
        is_diag = p == q
        sd = s[is_diag]
        draws[sd, p[is_diag], 0] = a[is_diag]         # z[p,p] = a + ib, then overwritten by a - ib (noise_model.py:196-199)
        low = p == q + 1                              # z[p][p-1] = a + ib: the lower element of bond p
        draws[s[low], p[low], 1] = a[low]
        draws[s[low], p[low], 2] = b[low]
        up = p == q - 1                               # z[p][p+1] = a + ib -> lower element z[q][p] = a - ib
        draws[s[up], q[up], 1] = a[up]
        draws[s[up], q[up], 2] = -b[up]
        if imag_off.any():
            draws[:, 1:, 2] += torch.as_tensor(imag_off, device=dev)
        ctrl_t = torch.as_tensor(ctrl, device=dev)
        fid = backend.mc_fidelity(ctrl_t, draws.view(C, K, n, 3), self.Nspin, self.inspin, self.outspin, h0_diag=diag,
                                  h0_offdiag=off, ring=ring)
        if sd.numel():
            imag = torch.zeros((sd.numel(), 1, n), dtype=torch.float64, device=dev)
            imag[torch.arange(sd.numel(), device=dev), 0, p[is_diag]] = -b[is_diag]
            sub = backend.mc_fidelity_nonhermitian(ctrl_t[sd // K], draws[sd][:, None], imag, self.Nspin, self.inspin,
                                                   self.outspin, h0_diag=diag, h0_offdiag=off, ring=ring)
            fid.view(-1)[sd] = sub[:, 0]
        return self._to_host(fid)

    def _to_host(self, fid) -> np.ndarray:
        """(C, K) device tensor -> NumPy through a pinned staging buffer kept on the instance (pageable D2H of 8 MB runs at
        a third of the pinned rate)."""
        import torch
        # torch's caching HOST allocator: the block comes from its pool after the first call, belongs to the returned array
        # (numpy keeps the tensor alive) and goes back to the pool with it - no staging copy (8 MB: 0.35 ms of memcpy)
        host = torch.empty(fid.shape, dtype=torch.float64, pin_memory=True)
        host.copy_(fid, non_blocking=True)
        torch.cuda.current_stream(fid.device).synchronize()
        return host.numpy()
