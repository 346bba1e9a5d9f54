"""Host-side wrappers over the C ABI (include/robchar_hip.h): NumPy arrays or torch CUDA tensors in,
same kind out.  One call = one sigma_sim level = C x K evaluations of the reference's
`evaluate_noisy_fidelity(x, ham_noisy=True)` (noise_model.py:98-109), or the per-controller metric
reductions of mcsim.py:144-183 / :480-500.

NumPy path : blocking `rc_mc_fidelity_f64` / `rc_reduce_f64` (host buffers staged by the library).
torch path : `*_async` entry points on torch's CURRENT stream with device pointers - nothing is copied and
             nothing synchronises; torch is used only as the owner of device memory and streams.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

Q_THRESHOLDS = (0.95, 0.98)          # mcsim.py:179-180


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


# ---- argument marshalling: each piece of an entry's argument list is made in ONE place, the helpers from here to `_outputs`
def _np_f64(a, shape=None, name="array"):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {a.shape}")
    return a


def _ptr(a):
    """Address of a NumPy array for the C ABI (None -> NULL)."""
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _dev_ptr(t):
    """Address of a torch tensor's first element for the C ABI (None -> NULL)."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _on_stream(dev):
    """(device index, stream) - the two leading arguments of every `*_async` entry: torch's CURRENT stream on `dev`."""
    import torch
    return dev.index or 0, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


_f64 = None                          # torch.float64 once a CUDA tensor has been seen (this module imports without torch)


def _is_dev_f64(t, shape=None) -> bool:
    """Is `t` a contiguous float64 CUDA tensor (of the shape in this tuple, when one is given)?  (Only a tensor has `is_cuda`.)"""
    global _f64
    if not getattr(t, "is_cuda", False):
        return False
    if _f64 is None:
        import torch
        _f64 = torch.float64
    return t.dtype == _f64 and t.is_contiguous() and (shape is None or t.shape == shape)


def _check_geometry(nspin, inspin, outspin):
    if not (2 <= int(nspin) <= 32):
        raise ValueError("Nspin must be in [2, 32]")
    if not (0 <= int(inspin) < nspin and 0 <= int(outspin) < nspin):
        raise ValueError("inspin/outspin out of range")


def _check_want(want, outputs, allow_empty=False):
    want = tuple(want)
    if not (want or allow_empty) or any(w not in outputs for w in want):
        raise ValueError(f"want: a {'' if allow_empty else 'non-empty '}subset of {outputs}, got {want}")
    return want


def _static_terms(h0_diag, h0_offdiag, nspin):
    """The static Hamiltonian's (N,) diagonal and (N - 1,) couplings as float64 vectors (None stays None -> NULL)."""
    return (None if h0_diag is None else _np_f64(h0_diag, (nspin,), "h0_diag"),
            None if h0_offdiag is None else _np_f64(h0_offdiag, (nspin - 1,), "h0_offdiag"))


def _draw_args(controllers, draws, nspin):
    """A draw tensor beside its controllers -> (draws, C, K, shared, stride): draws (C, K, N, 3), or (1, K, N, 3) with C > 1
    controllers = ONE set for every controller (`shared`); `stride` is the `draws_ctrl_stride` of the C entries, 0 when shared."""
    C = controllers.shape[0] if hasattr(controllers, "shape") else len(controllers)
    if not hasattr(draws, "shape"):
        draws = np.asarray(draws, dtype=np.float64)
    shape = draws.shape
    shared = len(shape) == 4 and shape[0] == 1 and C > 1
    if len(shape) != 4 or shape != ((1 if shared else C), shape[1], nspin, 3):
        raise ValueError(f"draws: expected ({C}, K, {nspin}, 3) for the {C} controllers, or (1, K, {nspin}, 3), got {tuple(shape)}")
    K = shape[1]
    return draws, C, K, shared, (0 if shared else K * nspin * 3)


def _controllers_on(controllers, dev, C, nspin):
    """The controllers as the contiguous float64 (C, N+1) tensor on `dev` (rows that are not a tensor are uploaded)."""
    import torch
    ctrl = controllers if _is_torch(controllers) else torch.as_tensor(np.asarray(controllers, dtype=np.float64))
    ctrl = ctrl.to(device=dev, dtype=torch.float64).contiguous()
    if tuple(ctrl.shape) != (C, nspin + 1):
        raise ValueError(f"controllers: expected ({C}, {nspin + 1}), got {tuple(ctrl.shape)}")
    return ctrl


def _shared_draws_via_torch(call, controllers, draws, device):
    """A NumPy call with ONE shared (1, K, N, 3) draw set: that form exists on the enqueue path only, so both arrays are uploaded
    to GPU `device`, `call(controllers, draws)` runs the torch path, and its tensor (or dict of tensors) comes back as NumPy."""
    import torch
    dev = torch.device("cuda", device)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    res = call(up(controllers), up(draws))
    return {k: v.cpu().numpy() for k, v in res.items()} if isinstance(res, dict) else res.cpu().numpy()


def _generated_draws_args(controllers, n_draws, sigma, seed, offset, nspin):
    """The arguments of an entry that generates its draws inside the kernel -> (ctrl, rows, C, K, draw_args): `ctrl` the
    controllers as a contiguous float64 (C, N+1) CUDA tensor (a NumPy array is uploaded to the current device), `rows` the (C,)
    per-row scales on its device or None for a float `sigma`, `draw_args` the entry's (seed, offset, sigma, sigma_rows).
    Everything is validated BEFORE the library is loaded; the caller keeps `ctrl` and `rows` until the entry has returned."""
    upload = not _is_torch(controllers)
    if upload:
        controllers = np.ascontiguousarray(controllers, dtype=np.float64)
    shape = controllers.shape
    if len(shape) != 2 or shape[1] != nspin + 1:
        raise ValueError(f"controllers: expected (C, {nspin + 1}), got {tuple(shape)}")
    C, K = shape[0], int(n_draws)
    if K < 0:
        raise ValueError("n_draws must be non-negative")
    per_row = not isinstance(sigma, (int, float)) and np.ndim(sigma) > 0
    if per_row:
        if not _is_torch(sigma):
            sigma = np.ascontiguousarray(sigma, dtype=np.float64)
        if tuple(sigma.shape) != (C,):
            raise ValueError("sigma: a float or a (C,) tensor")
    _lib.load()
    _lib.require_gpu()
    if upload:                                       # (NumPy rows are uploaded to the current device; the results stay there)
        import torch
        controllers = torch.from_numpy(controllers).to(compute_device())
    if not controllers.is_cuda:
        raise ValueError("controllers must be a torch CUDA tensor (or a NumPy array, which is uploaded)")
    ctrl = controllers.double().contiguous()
    rows = None
    if per_row:
        import torch
        rows = (sigma if _is_torch(sigma) else torch.from_numpy(sigma)).to(device=ctrl.device, dtype=torch.float64).contiguous()
    return ctrl, rows, C, K, (int(seed) & (2 ** 64 - 1), int(offset), 0.0 if per_row else float(sigma), _dev_ptr(rows))


def _outputs(outputs, want, shapes, dev=None, dtypes=None):
    """Allocate the outputs named in `want` (in that order) with `shapes[name]`: torch tensors on `dev` (float64, or
    `dtypes[name]`), NumPy float64 arrays for dev = None -> (the dict, the pointers in the order of `outputs`: NULL = not asked for)."""
    if dev is None:
        res = {k: np.empty(shapes[k], dtype=np.float64) for k in want}
        return res, [_ptr(res.get(k)) for k in outputs]
    import torch
    res = {k: torch.empty(shapes[k], dtype=(dtypes or {}).get(k, torch.float64), device=dev) for k in want}
    return res, [_dev_ptr(res.get(k)) for k in outputs]


def compute_device():
    """torch.device of the GPU this process computes on: torch's CURRENT device (one process per GPU sets it with
    `torch.cuda.set_device(LOCAL_RANK)`); raises when no GPU is visible (there is no CPU path)."""
    _lib.require_gpu()
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def device_index(device=None) -> int:
    """Device ordinal for the C ABI: an explicit int / torch.device, else torch's current device (0 before torch has
    been imported by anybody: the plain-ctypes use of the library)."""
    if device is None:
        import sys
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_available():
            return int(torch.cuda.current_device())
        return 0
    if isinstance(device, int):
        return device
    return int(device.index or 0)


# metric rows of a slab packed into one (15, R) tensor: rim1[3] std[3] min[3] q[3][2]  (variant order: centre, upper, lower)
PACKED_ROWS = 15


def packed_views(packed):
    """The (15, R) packed metric tensor as the dict of views `reduce_metrics(out=...)` fills."""
    R = packed.shape[1]
    return {"rim1": packed[0:3], "std": packed[3:6], "min": packed[6:9], "q": packed[9:15].view(3, 2, R)}


def reduce_packed(fid2d, dkw_eps: float, out=None, overlapped: bool = True):
    """`reduce_metrics` of an (R, K) device slab with the reference's two thresholds into ONE (15, R) tensor - the
    only thing a metrics-only caller has to move to the host (120 bytes per controller row).  `overlapped`: see
    `reduce_metrics`."""
    import torch
    R = int(fid2d.shape[0])
    if out is None:
        out = torch.empty((PACKED_ROWS, R), dtype=torch.float64, device=fid2d.device)
    if R:
        reduce_metrics(fid2d, dkw_eps=dkw_eps, out=packed_views(out), overlapped=overlapped)
    return out


def mc_fidelity(controllers, draws, nspin: int, inspin: int, outspin: int, h0_diag=None, h0_offdiag=None,
                ring: bool = False, device=None, kernel: str = "auto", out=None):
    """Fidelities |<out| exp(-i T H) |in>|^2 for C controllers x K perturbations.

    controllers (C, N+1); draws (C, K, N, 3) already scaled by sigma -> (C, K).  draws of shape (1, K, N, 3)
    with C > 1 controllers = ONE set of K perturbations applied to every controller (the fixed Hamiltonian sets of
    the reference's optimiser-side objective, qnewton.py:122-137, :426-444).
    NumPy inputs -> NumPy output (blocking).  torch CUDA tensors -> torch tensor on the same device,
    enqueued on the current stream (asynchronous).
    """
    _check_geometry(nspin, inspin, outspin)
    lib = _lib.load()
    _lib.require_gpu()
    device = device_index(device)
    h0d, h0o = _static_terms(h0_diag, h0_offdiag, nspin)
    kid = _lib.KERNELS[kernel]
    draws, C, K, shared, stride = _draw_args(controllers, draws, nspin)
    if _is_torch(draws):
        import torch
        if not _is_dev_f64(draws):
            raise ValueError("draws must be a contiguous float64 CUDA tensor")
        dev = draws.device
        ctrl = _controllers_on(controllers, dev, C, nspin)
        if out is None:
            out = torch.empty((C, K), dtype=torch.float64, device=dev)
        elif not _is_dev_f64(out, (C, K)):
            raise ValueError("out must be a contiguous float64 CUDA tensor of shape (C, K)")
        _lib.check(lib.rc_mc_fidelity_ex_f64_async(    # (`_on_stream` spelled out: its call is measurable in bench.py's timed loop)
            dev.index or 0, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), kid, nspin, inspin, outspin, _ptr(h0d), _ptr(h0o),
            int(bool(ring)), _dev_ptr(ctrl), _dev_ptr(draws), stride, C, K, _dev_ptr(out)))
        return out
    if shared:
        res = _shared_draws_via_torch(lambda c, d: mc_fidelity(c, d, nspin, inspin, outspin, h0_diag=h0_diag, h0_offdiag=h0_offdiag,
                                                               ring=ring, kernel=kernel), controllers, draws, device)
        if out is not None:
            out[...] = res
            return out
        return res
    draws = np.ascontiguousarray(draws, dtype=np.float64)
    ctrl = _np_f64(controllers, (C, nspin + 1), "controllers")
    res = np.empty((C, K), dtype=np.float64) if out is None else out
    _lib.check(lib.rc_mc_fidelity_kernel_f64(device, kid, nspin, inspin, outspin, _ptr(h0d), _ptr(h0o), int(bool(ring)),
                                             _ptr(ctrl), _ptr(draws), C, K, _ptr(res)))
    return res


GRAD_OUTPUTS = ("fid", "grad", "mean")


def max_nspin_grad() -> int:
    """`RC_MAX_NSPIN_GRAD` of include/robchar_hip.h: the longest chain the gradient kernel takes"""
    return 12


def mc_fidelity_grad(controllers, draws, nspin: int, inspin: int, outspin: int, h0_diag=None, h0_offdiag=None,
                     device=None, want=GRAD_OUTPUTS):
    """Fidelities and their gradient with respect to the controller rows x = [B_0 .. B_{N-1}, T] (chain topology,
    N <= `max_nspin_grad()`), in one kernel launch.  Returns a dict with the entries named in `want`:

        "fid"  (C, K)         the fidelities (agree with `mc_fidelity` to rounding, not bit for bit: another eigensolver route)
        "grad" (C, K, N + 1)  dF/dx_0 .. dF/dx_{N-1}, dF/dx_N = sign(x_N) dF/dT, per sample
        "mean" (C, N + 2)     (mean F, mean dF/dx_0 .. mean dF/dx_N) over the K samples of each row; deterministic

    Shapes and the NumPy / torch convention as in `mc_fidelity`: NumPy in -> NumPy out (blocking); torch CUDA tensors ->
    tensors on the same device, enqueued on the current stream; draws of shape (1, K, N, 3) with C > 1 = ONE draw set for
    every controller (the optimiser-side objective `fidelity_ss_av` and its gradient).  A NaN controller row gives NaN."""
    return _fidelity_derivatives("grad", GRAD_OUTPUTS, lambda C, K, N: {"fid": (C, K), "grad": (C, K, N + 1), "mean": (C, N + 2)},
                                 controllers, draws, nspin, inspin, outspin, h0_diag, h0_offdiag, device, want)


def _fidelity_derivatives(which, outputs, shapes_of, controllers, draws, nspin, inspin, outspin, h0_diag, h0_offdiag, device, want,
                          ring_args=(), late_args=None, shared_via_torch=None):
    """`mc_fidelity_grad` (which = "grad"), `mc_fidelity_sens` ("sens") and `mc_fidelity_times` ("times"): the C entries
    `rc_mc_fidelity_<which>_f64[_async]` differ in their outputs, in `ring_args`, which the entry takes between `h0_offdiag` and
    the controllers, and in `late_args(dev)` -> (what it takes between `K` and the outputs for tensors on `dev`, or host arrays
    for dev = None; whatever has to outlive the call).  `shared_via_torch`: where the blocking entry is not used for one shared
    draw set, the torch call that takes its place (`_shared_draws_via_torch`).  Geometry, `want`, the static terms and the draws'
    shape are validated before the library is loaded."""
    _check_geometry(nspin, inspin, outspin)
    want = _check_want(want, outputs)
    h0d, h0o = _static_terms(h0_diag, h0_offdiag, nspin)
    draws, C, K, shared, stride = _draw_args(controllers, draws, nspin)
    lib = _lib.load()
    _lib.require_gpu()
    device = device_index(device)
    if late_args is None:
        late_args = lambda dev: ((), None)           # (the second item: the tensors behind the pointers in the first)
    if _is_torch(draws):
        if not _is_dev_f64(draws):
            raise ValueError("draws must be a contiguous float64 CUDA tensor")
        dev = draws.device
        ctrl = _controllers_on(controllers, dev, C, nspin)
        late, keep = late_args(dev)
        res, out_ptr = _outputs(outputs, want, shapes_of(C, K, nspin), dev)
        _lib.check(getattr(lib, f"rc_mc_fidelity_{which}_f64_async")(
            *_on_stream(dev), nspin, inspin, outspin, _ptr(h0d), _ptr(h0o), *ring_args, _dev_ptr(ctrl), _dev_ptr(draws), stride, C, K,
            *late, *out_ptr))
        return res
    if shared and shared_via_torch is not None:
        return _shared_draws_via_torch(shared_via_torch, controllers, draws, device)
    draws = np.ascontiguousarray(draws, dtype=np.float64)
    ctrl = _np_f64(controllers, (C, nspin + 1), "controllers")
    late, keep = late_args(None)
    res, out_ptr = _outputs(outputs, want, shapes_of(C, K, nspin))
    _lib.check(getattr(lib, f"rc_mc_fidelity_{which}_f64")(
        device, nspin, inspin, outspin, _ptr(h0d), _ptr(h0o), *ring_args, _ptr(ctrl), _ptr(draws), stride, C, K, *late, *out_ptr))
    return res


def _tile_counter(symbol_name, device, reset) -> int:
    """One of the library's diagnostic tile counters (`rc_stats_*_tiles`), optionally zeroed behind the read."""
    n = int(getattr(_lib.load(), symbol_name)(device_index(device), int(bool(reset))))
    if n < 0:
        _lib.check(n)
    return n


def grad_general_tiles(device=None, reset: bool = False) -> int:
    """Tiles of the gradient kernel in which some sample took the textbook per-sample QL since the last reset (diagnostic)."""
    return _tile_counter("rc_stats_grad_general_tiles", device, reset)


SENS_OUTPUTS = ("fid", "sens", "mean")


def mc_fidelity_sens(controllers, draws, nspin: int, inspin: int, outspin: int, h0_diag=None, h0_offdiag=None,
                     device=None, want=SENS_OUTPUTS):
    """Fidelities and their derivatives with respect to the structured noise - the samples' own draws g (chain topology,
    N <= `max_nspin_grad()`), in one kernel launch.  Returns a dict with the entries named in `want`:

        "fid"  (C, K)         the fidelities (as in `mc_fidelity_grad`)
        "sens" (C, K, N, 3)   dF/dg in the draws' layout: [i][0] site energy i, [i][1] / [i][2] real / imaginary part of the coupling
                              of the sites i - 1 and i; [0][1] = [0][2] = 0.  Exactly 0 for both parts of an exactly cut bond
        "mean" (C, 3 N + 2)   (mean F, mean rho, the N x 3 mean dF/dg) over the K samples of each row, rho = sum g dF/dg: for draws
                              g = sigma z the mean rho is dFbar/dln(sigma) at that sigma; deterministic

    Shapes, the NumPy / torch convention, the shared draw set (1, K, N, 3) and NaN rows as in `mc_fidelity_grad`."""
    return _fidelity_derivatives("sens", SENS_OUTPUTS, lambda C, K, N: {"fid": (C, K), "sens": (C, K, N, 3), "mean": (C, 3 * N + 2)},
                                 controllers, draws, nspin, inspin, outspin, h0_diag, h0_offdiag, device, want)


def sens_general_tiles(device=None, reset: bool = False) -> int:
    """Tiles of the sensitivity kernel in which some sample took the textbook per-sample QL since the last reset (diagnostic)."""
    return _tile_counter("rc_stats_sens_general_tiles", device, reset)


TIMES_OUTPUTS = ("fid", "wsum", "min")
MAX_TIMES = 64                       # RC_MAX_TIMES of include/robchar_hip.h
MAX_NSPIN_TIMES = 16                 # RC_MAX_NSPIN_FAST


def readout_times(T, tscale=None, tshift=None):
    """The (C, M) readout times t_cj = |T_c tscale_j + tshift_j| the readout-time kernels evaluate: NumPy's product, then sum,
    then absolute value - the kernels' own rounding, bit for bit.  `T`: the controllers' time entries as stored (signed); an
    absent array is all 1 / all 0; with both absent M = 1."""
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    a, b, _ = _times_grid(tscale, tshift, None)
    return np.abs(T[:, None] * a[None, :] + b[None, :])


def _times_grid(tscale, tshift, weights):
    """(tscale, tshift, weights) as float64 NumPy vectors of one length M in 1 .. MAX_TIMES; an absent scale / shift is filled
    with 1 / 0, absent weights stay None."""
    vec = lambda v: None if v is None else np.ascontiguousarray(
        v.detach().cpu().numpy() if _is_torch(v) else v, dtype=np.float64).reshape(-1)
    a, b, w = vec(tscale), vec(tshift), vec(weights)
    lens = {len(v) for v in (a, b, w) if v is not None}
    if len(lens) > 1:
        raise ValueError(f"tscale, tshift and weights must have one length, got {sorted(lens)}")
    M = lens.pop() if lens else 1
    if not (1 <= M <= MAX_TIMES):
        raise ValueError(f"the grid must hold 1 .. {MAX_TIMES} times, got {M}")
    return (np.ones(M) if a is None else a), (np.zeros(M) if b is None else b), w


_TIMES_GRIDS = {}                   # (device, grid bytes) -> (3, M) device tensor: tscale, tshift, weights (zeros when absent)


def _times_grid_on_device(a, b, w, dev):
    """The grid as one (3, M) tensor on `dev`, uploaded once per distinct grid (a blocking copy: it has landed when this returns,
    so the tensor may be read from any stream) and kept - a caller that sweeps controllers over one grid pays no copy per call."""
    import torch
    key = (str(dev), a.tobytes(), b.tobytes(), None if w is None else w.tobytes())
    grid = _TIMES_GRIDS.get(key)
    if grid is None:
        if len(_TIMES_GRIDS) >= 16:
            _TIMES_GRIDS.clear()
        grid = torch.from_numpy(np.stack([a, b, w if w is not None else np.zeros(len(a))])).to(dev)
        _TIMES_GRIDS[key] = grid
    return grid


def _times_want(want, weights, nspin, inspin, outspin):
    _check_geometry(nspin, inspin, outspin)
    if nspin > MAX_NSPIN_TIMES:
        raise ValueError(f"the readout-time kernels support chains of N <= {MAX_NSPIN_TIMES} spins")
    want = _check_want(want, TIMES_OUTPUTS)
    if "wsum" in want and weights is None:
        raise ValueError("want 'wsum' needs weights")
    return want


def _times_args(a, b, w):
    """The readout-time entries' own arguments: the outputs' shapes, and the `late_args` between `K` and the outputs - M and the
    grid's three pointers (NULL weights when absent), host arrays for dev = None, else the grid's tensor on `dev`."""
    M = len(a)

    def late_args(dev):
        if dev is None:
            return (M, _ptr(a), _ptr(b), _ptr(w)), (a, b, w)
        grid = _times_grid_on_device(a, b, w, dev)
        return (M, _dev_ptr(grid[0]), _dev_ptr(grid[1]), _dev_ptr(grid[2]) if w is not None else None), grid
    return (lambda C, K, N: {"fid": (M, C, K), "wsum": (C, K), "min": (C, K)}), late_args


def mc_fidelity_times(controllers, draws, nspin: int, inspin: int, outspin: int, tscale=None, tshift=None, weights=None,
                      want=("fid",), h0_diag=None, h0_offdiag=None, device=None):
    """Fidelities on a grid of M readout times from ONE eigen decomposition per sample (`rc_mc_fidelity_times_f64[_async]`; chain
    topology, N <= 16, any (in, out)): F_j(c, k) = |<out| exp(-i H_ck t_cj) |in>|^2 at t_cj = `readout_times(T, tscale, tshift)`.
    Returns a dict with the entries named in `want`:

        "fid"  (M, C, K)   M slabs, each what `mc_fidelity(kernel="tridiag_ql")` gives for controllers whose time entry is t_cj,
                           bit for bit: `reduce_metrics`, `bootstrap_metrics`, `tail_select` take slab j unchanged
        "wsum" (C, K)      acc = weights[0] F_0; acc = fma(weights[j], F_j, acc) in the order of j (needs `weights`)
        "min"  (C, K)      min_j F_j

    `tscale`, `tshift`, `weights`: (M,) arrays, 1 <= M <= 64; an absent scale / shift is all 1 / all 0.  Shapes and the
    NumPy / torch convention as in `mc_fidelity`: NumPy in -> NumPy out (blocking); torch CUDA draws -> tensors on the same device,
    enqueued on the current stream; draws of shape (1, K, N, 3) with C > 1 = ONE draw set for every controller.  A NaN controller
    row gives NaN in every output."""
    want = _times_want(want, weights, nspin, inspin, outspin)
    a, b, w = _times_grid(tscale, tshift, weights)
    shapes_of, late_args = _times_args(a, b, w)
    via_torch = lambda c, d: mc_fidelity_times(c, d, nspin, inspin, outspin, tscale=a, tshift=b, weights=w, want=want,
                                               h0_diag=h0_diag, h0_offdiag=h0_offdiag)
    return _fidelity_derivatives("times", TIMES_OUTPUTS, shapes_of, controllers, draws, nspin, inspin, outspin, h0_diag, h0_offdiag,
                                 device, want, ring_args=(0,), late_args=late_args, shared_via_torch=via_torch)


def mc_fidelity_times_philox(controllers, n_draws: int, nspin: int, inspin: int, outspin: int, seed: int, offset: int = 0,
                             sigma=0.05, tscale=None, tshift=None, weights=None, want=("fid",), h0_diag=None, h0_offdiag=None):
    """`mc_fidelity_times` with the counter-based draws generated INSIDE the kernel (`rc_mc_fidelity_times_philox_f64_async`):
    controllers (C, N+1) torch CUDA tensor (a NumPy array is uploaded to the current device) -> dict of torch tensors on that
    device, the entries named in `want`, enqueued on the current stream; bit-identical to
    `mc_fidelity_times(controllers, philox_normal((C, K, N, 3), seed, scale=sigma, offset=offset), ...)` without that tensor.
    `sigma`: a float, or a (C,) tensor / array (one scale per controller row: every sigma level of an algorithm in one launch)."""
    want = _times_want(want, weights, nspin, inspin, outspin)
    shapes_of, late_args = _times_args(*_times_grid(tscale, tshift, weights))
    return _fidelity_derivatives_philox("times_philox", TIMES_OUTPUTS, shapes_of, controllers, n_draws, nspin, inspin, outspin, seed,
                                        offset, sigma, h0_diag, h0_offdiag, want, ring_args=(0,), late_args=late_args)


def times_general_tiles(device=None, reset: bool = False) -> int:
    """Tiles of the readout-time kernels in which some sample took the textbook per-sample QL since the last reset (diagnostic)."""
    return _tile_counter("rc_stats_times_general_tiles", device, reset)


def reduce_metrics(fid, q_thresholds=Q_THRESHOLDS, dkw_eps: float = 0.0, want_sorted: bool = False,
                   device=None, out=None, overlapped: bool = True):
    """Per-controller reductions of a (C, K) fidelity slab on the GPU.

    Returns a dict of arrays with a leading variant axis of length 3 (0 centre, 1 " upper" = clip(F-eps),
    2 " lower" = clip(F+eps); mcsim.py:484-485):  rim1 (3,C) = W1 to delta(x-1) = mean infidelity,
    std (3,C), min (3,C), q (3,nq,C) = fraction >= threshold (positive; the reference stores -q), and
    optionally sorted (C,K).  `out` (torch path): dict of preallocated outputs to reuse across calls.
    `overlapped` (torch path; the NumPy path is blocking and always standalone): does the caller run fidelity launches on
    another stream BESIDE this reduction?  False = nothing overlaps it (`RC_REDUCE_STANDALONE`: rows of 8193 .. 10 240 values
    take the dense route, 2x faster alone; what `MCDataSim` passes); True = the latency-bound route that coexists with them
    (a pipelined caller like bench.py's steady state).  Only that row length is affected, and only in the last bits.
    """
    lib = _lib.load()
    _lib.require_gpu()
    thr = np.ascontiguousarray(q_thresholds, dtype=np.float64)
    nq = int(thr.size)
    if _is_torch(fid):
        import torch
        if not (_is_dev_f64(fid) and fid.dim() == 2):
            raise ValueError("fid must be a contiguous float64 CUDA tensor of shape (C, K)")
        C, K = (int(v) for v in fid.shape)
        dev = fid.device
        mk = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
        if out is not None:          # caller-provided contiguous float64 CUDA buffers (torch path only)
            res = {k: out[k] for k in ("rim1", "std", "min", "q")}
            assert _is_dev_f64(res["rim1"], (3, C)) and _is_dev_f64(res["q"], (3, max(nq, 1), C))
            assert _is_dev_f64(res["std"]) and _is_dev_f64(res["min"])
        else:
            res = {"rim1": mk(3, C), "std": mk(3, C), "min": mk(3, C), "q": mk(3, max(nq, 1), C)}
        srt = mk(C, K) if want_sorted else None
        _lib.check(lib.rc_reduce_ex_f64_async(         # (`_on_stream` spelled out, as in `mc_fidelity`)
            dev.index or 0, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), _dev_ptr(fid), C, K, _ptr(thr), nq,
            float(dkw_eps), _dev_ptr(res["rim1"]), _dev_ptr(res["std"]), _dev_ptr(res["min"]), _dev_ptr(res["q"]), _dev_ptr(srt),
            0 if overlapped else _lib.RC_REDUCE_STANDALONE))
        res["q"] = res["q"][:, :nq]
        if srt is not None:
            res["sorted"] = srt
        return res
    fid = np.ascontiguousarray(fid, dtype=np.float64)
    if fid.ndim != 2:
        raise ValueError("fid must have shape (C, K)")
    C, K = fid.shape
    device = device_index(device)
    res = {"rim1": np.empty((3, C)), "std": np.empty((3, C)), "min": np.empty((3, C)),
           "q": np.empty((3, nq, C))}
    srt = np.empty((C, K)) if want_sorted else None
    _lib.check(lib.rc_reduce_f64(device, _ptr(fid), C, K, _ptr(thr), nq, float(dkw_eps), _ptr(res["rim1"]),
                                 _ptr(res["std"]), _ptr(res["min"]), _ptr(res["q"]) if nq else None,
                                 _ptr(srt)))
    if srt is not None:
        res["sorted"] = srt
    return res


def rim_p(fid, p: float, device=None):
    """(mean_k (1 - f)^p)^(1/p) per row of a (C, K) slab on the GPU (wd_sortof_fast_implementation.py:147-174)."""
    lib = _lib.load()
    _lib.require_gpu()
    if _is_torch(fid):
        import torch
        if not (_is_dev_f64(fid) and fid.dim() == 2):
            raise ValueError("fid must be a contiguous float64 CUDA tensor of shape (C, K)")
        C, K = (int(v) for v in fid.shape)
        out = torch.empty((C,), dtype=torch.float64, device=fid.device)
        _lib.check(lib.rc_rim_p_f64_async(*_on_stream(fid.device), _dev_ptr(fid), C, K, float(p), _dev_ptr(out)))
        return out
    fid = np.ascontiguousarray(fid, dtype=np.float64)
    C, K = fid.shape
    out = np.empty((C,))
    _lib.check(lib.rc_rim_p_f64(device_index(device), _ptr(fid), C, K, float(p), _ptr(out)))
    return out


def philox_normal(shape, seed: int, scale: float = 1.0, offset: int = 0, device=None, as_torch: bool = False, out=None):
    """sigma-scaled Gaussian draws from the device's counter-based generator (NOT the reference's RNG stream;
    see include/robchar_hip.h).  Element i of the flattened result is element `offset + i` of stream `seed`.
    Returns a NumPy array, or a torch CUDA tensor when `as_torch`."""
    lib = _lib.load()
    _lib.require_gpu()
    n = int(np.prod(shape))
    if as_torch or out is not None:
        import torch
        if out is not None:
            if not (_is_dev_f64(out) and out.numel() == n):
                raise ValueError("out must be a contiguous float64 CUDA tensor with prod(shape) elements")
            dev = out.device
        else:
            dev = torch.device("cuda", device_index(device)) if not hasattr(device, "type") else device
            out = torch.empty(tuple(shape), dtype=torch.float64, device=dev)
        _lib.check(lib.rc_draws_philox_f64_async(      # (`_on_stream` spelled out, as in `mc_fidelity`)
            dev.index or 0, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), int(seed), int(offset), n, float(scale), _dev_ptr(out)))
        return out
    out = np.empty(tuple(shape), dtype=np.float64)
    _lib.check(lib.rc_draws_philox_f64(device_index(device), int(seed), int(offset), n, float(scale), _ptr(out)))
    return out


_warned_log = []


def legacy_device_exact() -> bool:
    """Are the device-continued legacy normals NumPy's bit for bit on this host (`rc_legacy_log_is_host_exact`: the C library's
    log is the routine the device restates)?  When not, the callers below draw on the HOST instead - `legacy` mode means the
    reference's draws, not draws within a few ulp of them - and say so once."""
    ok = bool(_lib.load().rc_legacy_log_is_host_exact())
    if not ok and not _warned_log:
        _warned_log.append(1)
        import warnings
        warnings.warn("this host's libm log() is not the routine librobchar_hip.so restates on the device: legacy draws are "
                      "made by NumPy on the host (bit-identical, slower) instead of being continued on the GPU", RuntimeWarning)
    return ok


def legacy_stream_usable(rng) -> bool:
    """True when `rng` (a noise_function) draws from numpy's GLOBAL legacy stream with nothing but a scale - the
    reference's default generator (noise_model.py:114-115) - AND the device can continue that stream with NumPy's own
    normals (`legacy_device_exact`)."""
    return (getattr(rng, "generator", None) is np.random.normal and set(rng.args) <= {"scale", "loc"}
            and float(rng.args.get("loc", 0.0)) == 0.0 and legacy_device_exact())


def _legacy_state():
    """numpy's global legacy generator as the `rc_mt19937_state` the device continues."""
    name, key, pos, has_gauss, cached = np.random.get_state()
    if name != "MT19937":
        raise ValueError("numpy's global generator is not the legacy MT19937 stream")
    st = _lib.Mt19937State()
    ctypes.memmove(st.key, np.ascontiguousarray(key, dtype=np.uint32).ctypes.data, 624 * 4)
    st.pos, st.has_gauss, st.gauss = int(pos), int(has_gauss), float(cached)
    return st


def _set_legacy_state(st):
    np.random.set_state(("MT19937", np.frombuffer(st.key, dtype=np.uint32).copy(), int(st.pos), int(st.has_gauss), float(st.gauss)))


def legacy_normal_periods(n_periods: int, period: int, skip: int, scales, out=None, device=None):
    """Continue numpy's global legacy normal stream ON THE GPU (`rc_draws_legacy_f64`): `n_periods` periods of `period`
    draws, the first `skip` of each dropped (burned), the rest scaled by scales[p] -> torch tensor
    (n_periods, period - skip) on the device.  `np.random`'s state afterwards is exactly what the same draws through
    `np.random.normal` would have left (bit for bit), and so are the values wherever `legacy_device_exact()` holds (glibc's
    log restated on the device; a few ulp otherwise)."""
    import torch
    lib = _lib.load()
    _lib.require_gpu()
    scales = np.ascontiguousarray(scales, dtype=np.float64).reshape(-1)
    if scales.size != n_periods:
        raise ValueError("scales must have n_periods entries")
    if out is None:
        dev = torch.device("cuda", device_index(device))
        out = torch.empty((n_periods, period - skip), dtype=torch.float64, device=dev)
    elif not (_is_dev_f64(out) and out.numel() == n_periods * (period - skip)):
        raise ValueError("out must be a contiguous float64 CUDA tensor with n_periods * (period - skip) elements")
    st = _legacy_state()
    _lib.check(lib.rc_draws_legacy_f64(*_on_stream(out.device), ctypes.byref(st), int(n_periods), int(period), int(skip),
                                       _ptr(scales), _dev_ptr(out)))
    _set_legacy_state(st)
    return out


def directional_draws_device(n: int, ndir: int, sigma: float, device=None):
    """`n` samples of `directional_perturbation`'s RNG consumption (per sample `np.random.randint(0, ndir)` then two legacy
    normals scaled by sigma) continued from numpy's global legacy stream ON THE GPU (`rc_directional_draws_legacy_dev`)
    -> (idx int32 [n], ab float64 [n, 2]) torch CUDA tensors.  `np.random`'s state afterwards is what the n Python-level
    draws would have left, bit for bit; indices identical, normals identical where `legacy_device_exact()` holds."""
    import torch
    lib = _lib.load()
    _lib.require_gpu()
    dev = torch.device("cuda", device_index(device))
    idx = torch.empty((n,), dtype=torch.int32, device=dev)
    ab = torch.empty((n, 2), dtype=torch.float64, device=dev)
    if n == 0:
        return idx, ab
    st = _legacy_state()
    _lib.check(lib.rc_directional_draws_legacy_dev(*_on_stream(dev), ctypes.byref(st), int(n), int(ndir), float(sigma),
                                                   _dev_ptr(idx), _dev_ptr(ab)))
    _set_legacy_state(st)
    return idx, ab


def philox_fused_supported(nspin: int, ring: bool = False, kernel: str = "auto") -> bool:
    """Can `mc_fidelity_philox` take this geometry (chain, N <= 16, eigenvalue-only kernels)?"""
    return (not ring) and 2 <= nspin <= 16 and kernel in ("auto", "tridiag_adj")


def philox_fused_pays(nspin: int, inspin: int, outspin: int) -> bool:
    """Is the fused kernel the faster route for this geometry?  Measured at every size (profiles/r04_philox_fused_sweep.txt):
    0.70 - 0.86 of the two-kernel route's time up to N = 13 and for end-to-end pairs at N = 14; beyond that its instantiations
    run one wave per SIMD and generating the draw tensor first is 7 % faster.  (The results are bit-identical either way.)"""
    return bool(_lib.load().rc_philox_fused_pays(int(nspin), int(inspin), int(outspin)))


def mc_fidelity_philox(controllers, n_draws: int, nspin: int, inspin: int, outspin: int, seed: int, offset: int = 0,
                       sigma=0.05, h0_diag=None, h0_offdiag=None, kernel: str = "auto", out=None):
    """Fidelities with the counter-based draws generated INSIDE the kernel (`rc_mc_fidelity_philox_f64_async`): controllers
    (C, N+1) torch CUDA tensor -> (C, K) torch tensor on the same device, enqueued on the current stream; bit-identical to
    `mc_fidelity(controllers, philox_normal((C, K, N, 3), seed, scale=sigma, offset=offset))` without that tensor.
    `sigma`: a float, or a (C,) float64 CUDA tensor (one scale per controller row)."""
    import torch
    _check_geometry(nspin, inspin, outspin)
    if not getattr(controllers, "is_cuda", False):
        raise ValueError("controllers must be a torch CUDA tensor")
    if getattr(sigma, "ndim", 1) != 1 and _is_torch(sigma):      # (no 0-d tensor read as a float here: that would wait for the device)
        raise ValueError("sigma: a float or a (C,) tensor")
    h0d, h0o = _static_terms(h0_diag, h0_offdiag, nspin)
    ctrl, rows, C, K, draw_args = _generated_draws_args(controllers, n_draws, sigma, seed, offset, nspin)
    lib = _lib.load()
    dev = ctrl.device
    if out is None:
        out = torch.empty((C, K), dtype=torch.float64, device=dev)
    elif not _is_dev_f64(out, (C, K)):
        raise ValueError("out must be a contiguous float64 CUDA tensor of shape (C, K)")
    _lib.check(lib.rc_mc_fidelity_philox_f64_async(    # (`_on_stream` spelled out, as in `mc_fidelity`)
        dev.index or 0, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream), _lib.KERNELS[kernel], nspin, inspin, outspin,
        _ptr(h0d), _ptr(h0o), _dev_ptr(ctrl), *draw_args, C, K, _dev_ptr(out)))
    return out


def mc_fidelity_sens_philox(controllers, n_draws: int, nspin: int, inspin: int, outspin: int, seed: int, offset: int = 0,
                            sigma=0.05, h0_diag=None, h0_offdiag=None, want=SENS_OUTPUTS):
    """`mc_fidelity_sens` with the counter-based draws generated INSIDE the kernel (`rc_mc_fidelity_sens_philox_f64_async`):
    controllers (C, N+1) torch CUDA tensor (a NumPy array is uploaded to the current device) -> dict of torch tensors on that
    device ("fid" (C, K), "sens" (C, K, N, 3), "mean" (C, 3 N + 2), the entries named in `want`), enqueued on the current stream;
    bit-identical to
    `mc_fidelity_sens(controllers, philox_normal((C, K, N, 3), seed, scale=sigma, offset=offset))` without that tensor.
    `sigma`: a float, or a (C,) tensor / array (one scale per controller row: every sigma level of an algorithm in one launch).
    The mean rho in "mean"[:, 1] is taken over the generated draws sigma z: d fav / d ln(sigma) at the row's sigma; a
    row with sigma = 0 gives the nominal sensitivity with rho = 0.  Chain topology, N <= `max_nspin_grad()`."""
    return _fidelity_derivatives_philox("sens_philox", SENS_OUTPUTS, lambda C, K, N: {"fid": (C, K), "sens": (C, K, N, 3), "mean": (C, 3 * N + 2)},
                                        controllers, n_draws, nspin, inspin, outspin, seed, offset, sigma, h0_diag, h0_offdiag, want, ())


def _fidelity_derivatives_philox(which, outputs, shapes_of, controllers, n_draws, nspin, inspin, outspin, seed, offset, sigma,
                                 h0_diag, h0_offdiag, want, extra_args=(), late_args=None, ring_args=()):
    """`mc_fidelity_sens_philox` (which = "sens_philox"), `mc_fidelity_grad_philox` ("grad_philox"), `mc_fidelity_grad_listed`
    ("grad_listed") and `mc_fidelity_times_philox` ("times_philox"): the C entries differ in their outputs, in `ring_args`, which
    the entry takes between `h0_offdiag` and the controllers, in `extra_args`, which it takes between `sigma_rows` and `C`,
    and in `late_args(device)` -> (what it takes between `K` and the outputs, with tensors brought to the controllers' device;
    whatever has to outlive the call).  Everything is validated before the library is loaded."""
    _check_geometry(nspin, inspin, outspin)
    want = _check_want(want, outputs)
    h0d, h0o = _static_terms(h0_diag, h0_offdiag, nspin)
    ctrl, rows, C, K, draw_args = _generated_draws_args(controllers, n_draws, sigma, seed, offset, nspin)
    lib = _lib.load()
    dev = ctrl.device
    late, keep = late_args(dev) if late_args is not None else ((), None)     # (`keep`: the tensors behind the pointers in `late`)
    res, out_ptr = _outputs(outputs, want, shapes_of(C, K, nspin), dev)
    _lib.check(getattr(lib, f"rc_mc_fidelity_{which}_f64_async")(
        *_on_stream(dev), nspin, inspin, outspin, _ptr(h0d), _ptr(h0o), *ring_args, _dev_ptr(ctrl), *draw_args, *extra_args, C, K,
        *late, *out_ptr))
    return res


GRAD_PHILOX_OUTPUTS = ("fid", "grad", "mean", "moment")


def mc_fidelity_grad_philox(controllers, n_draws: int, nspin: int, inspin: int, outspin: int, seed: int, offset: int = 0,
                            sigma=0.05, shared: bool = False, h0_diag=None, h0_offdiag=None, want=GRAD_PHILOX_OUTPUTS):
    """`mc_fidelity_grad` with the counter-based draws generated INSIDE the kernel (`rc_mc_fidelity_grad_philox_f64_async`), and
    on request the second-moment sums behind the gradient of the row's variance: controllers (C, N+1) torch CUDA tensor (a NumPy
    array is uploaded to the current device) -> dict of torch tensors on that device, the entries named in `want`, enqueued on
    the current stream:

        "fid" (C, K), "grad" (C, K, N+1), "mean" (C, N+2) = (mean F, mean dF/dx)     as `mc_fidelity_grad`,
        "moment" (C, N+2) = (mean F^2, mean F dF/dx_0 .. mean F dF/dx_N)              (`noise.moments_from_sums`).

    Two draw modes.  shared=False: row c, draw k, site i, slot s is stream element offset + ((c K + k) N + i) 3 + s, and the first
    three outputs are bit-identical to `mc_fidelity_grad(controllers, philox_normal((C, K, N, 3), seed, scale=sigma, offset=offset))`.
    shared=True (common random numbers): the element is offset + (k N + i) 3 + s for every row - `mc_fidelity_grad` on the one set
    `philox_normal((1, K, N, 3), ...)`, bit for bit.  Neither tensor is ever built.
    `sigma`: a float, or a (C,) tensor / array (one scale per controller row); a row with sigma = 0 gives K identical samples.
    Chain topology, N <= `max_nspin_grad()`.  No automatic routing: DESIGN.md has the timing against the two-kernel route."""
    return _fidelity_derivatives_philox("grad_philox", GRAD_PHILOX_OUTPUTS,
                                        lambda C, K, N: {"fid": (C, K), "grad": (C, K, N + 1), "mean": (C, N + 2), "moment": (C, N + 2)},
                                        controllers, n_draws, nspin, inspin, outspin, seed, offset, sigma, h0_diag, h0_offdiag, want,
                                        (int(bool(shared)),))


def mc_fidelity_grad_times_philox(controllers, n_draws: int, nspin: int, inspin: int, outspin: int, seed: int, offset: int = 0,
                                  sigma=0.05, shared: bool = False, tscale=None, tshift=None, weights=None, h0_diag=None,
                                  h0_offdiag=None, want=GRAD_PHILOX_OUTPUTS):
    """`mc_fidelity_grad_philox` on a GRID OF READOUT TIMES from ONE eigen decomposition per sample
    (`rc_mc_fidelity_grad_times_philox_f64_async`): with u_cj = T_c tscale_j + tshift_j (|u_cj| = `readout_times`) and the
    weights w_j, per sample W = sum_j w_j F(u_cj) and its gradient with respect to the controller row,

        "fid" (C, K) = W, "grad" (C, K, N+1) = dW/dx  (the time entry: sum_j w_j tscale_j sgn(u_cj) F'(|u_cj|)),
        "mean" (C, N+2) = (mean W, mean dW/dx), "moment" (C, N+2) = (mean W^2, mean W dW/dx)   (`noise.moments_from_sums`),

    the entries named in `want`, torch tensors on the controllers' device, enqueued on the current stream.  `tscale`, `tshift`:
    (M,) arrays, absent = all 1 / all 0; `weights`: (M,), required; 1 <= M <= 64 - `noise.readout_jitter_nodes` makes the grid of
    Gaussian readout jitter.  The grid is uploaded once per distinct grid.  "fid" and "grad" are bit for bit what M calls of
    `mc_fidelity_grad_philox` on controllers with the time entry u_cj give, the time column multiplied by tscale_j and the slabs
    combined by acc = w_0 v_0; acc = fma(w_j, v_j, acc).  Draw modes, `sigma`, NaN rows, N <= `max_nspin_grad()`: as there."""
    if weights is None:
        raise ValueError("weights: required (one per grid time)")
    a, b, w = _times_grid(tscale, tshift, weights)
    M = len(a)

    def late_args(dev):
        grid = _times_grid_on_device(a, b, w, dev)
        return (M, _dev_ptr(grid[0]), _dev_ptr(grid[1]), _dev_ptr(grid[2])), grid

    return _fidelity_derivatives_philox("grad_times_philox", GRAD_PHILOX_OUTPUTS,
                                        lambda C, K, N: {"fid": (C, K), "grad": (C, K, N + 1), "mean": (C, N + 2), "moment": (C, N + 2)},
                                        controllers, n_draws, nspin, inspin, outspin, seed, offset, sigma, h0_diag, h0_offdiag, want,
                                        (int(bool(shared)),), late_args)


GRAD_LISTED_OUTPUTS = ("fid", "grad", "sum")


def mc_fidelity_grad_listed(controllers, n_draws: int, listed, weights=None, *, nspin: int, inspin: int, outspin: int, seed: int,
                            offset: int = 0, sigma=0.05, shared: bool = False, h0_diag=None, h0_offdiag=None,
                            want=GRAD_LISTED_OUTPUTS):
    """`mc_fidelity_grad_philox` over a chosen LIST of each row's `n_draws` draws, with weights on the row sums
    (`rc_mc_fidelity_grad_listed_f64_async`): only the listed samples are computed.  controllers (C, N+1) torch CUDA tensor (a NumPy
    array is uploaded); `listed` (C, L) int32 CUDA tensor (an integer NumPy array is uploaded): slot s of row c is draw
    k = listed[c, s] of that row - the stream element offset + ((c K + k) N + i) 3 + s', with shared=True offset + (k N + i) 3 + s' -,
    a value outside 0 .. K - 1 an EMPTY slot, repeats allowed; `weights` (C, L) float64 or None (= 1).  -> dict of torch tensors on
    the controllers' device, the entries named in `want`, enqueued on the current stream:

        "fid" (C, L), "grad" (C, L, N+1)      per slot, NaN in an empty slot,
        "sum" (C, N+2) = sum_s weights[c, s] (F, dF/dx)(c, listed[c, s])             fixed order, no atomics: same inputs, same bits.

    A sample's bits depend on (c, k) and the other arguments only - not on L, the slot or what else is listed.  Against
    `mc_fidelity_grad_philox` on all K draws they agree to rounding, not bit for bit (there the wave votes the QL sweep counts).
    `noise.tail_weights` makes the list and weights of CVaR_alpha.  `sigma`, NaN rows, chain topology, N <= `max_nspin_grad()`: as
    `mc_fidelity_grad_philox`."""
    if _is_torch(listed):
        import torch
        if listed.dtype != torch.int32:
            raise ValueError("listed: an int32 tensor")
    else:
        listed = np.asarray(listed)
        if listed.dtype.kind not in "iu":
            raise ValueError("listed: an integer array")
        listed = np.ascontiguousarray(listed, dtype=np.int32)
    nrows = int(controllers.shape[0]) if hasattr(controllers, "shape") else len(controllers)
    if listed.ndim != 2 or int(listed.shape[0]) != nrows:
        raise ValueError(f"listed: expected ({nrows}, L), got {tuple(listed.shape)}")
    L = int(listed.shape[1])
    if weights is not None:
        if not _is_torch(weights):
            weights = np.ascontiguousarray(weights, dtype=np.float64)
        elif str(weights.dtype) != "torch.float64":
            raise ValueError("weights: a float64 tensor")
        if tuple(weights.shape) != (nrows, L):
            raise ValueError(f"weights: expected {(nrows, L)}, got {tuple(weights.shape)}")

    def late_args(dev):
        import torch
        lst = (listed if _is_torch(listed) else torch.from_numpy(listed)).to(device=dev).contiguous()
        wts = None if weights is None else (weights if _is_torch(weights) else torch.from_numpy(weights)).to(device=dev).contiguous()
        return (_dev_ptr(lst), _dev_ptr(wts), L), (lst, wts)

    res = _fidelity_derivatives_philox("grad_listed", GRAD_LISTED_OUTPUTS,
                                       lambda C, K, N: {"fid": (C, L), "grad": (C, L, N + 1), "sum": (C, N + 2)},
                                       controllers, n_draws, nspin, inspin, outspin, seed, offset, sigma, h0_diag, h0_offdiag, want,
                                       (int(bool(shared)),), late_args)
    if int(n_draws) == 0 or L == 0:                  # (the entry writes nothing then: every slot is empty)
        for k, v in res.items():
            v.fill_(0.0 if k == "sum" else float("nan"))
    return res


TAIL_SELECT_OUTPUTS = ("list", "weight", "var")


def tail_select_len(n_draws: int, alpha: float) -> int:
    """m = min(K, ceil(alpha K)) as the library computes it (`rc_tail_select_len`, host only)."""
    m = int(_lib.load().rc_tail_select_len(int(n_draws), float(alpha)))
    if m < 0:
        raise ValueError("alpha must be in (0, 1] and n_draws in 0 .. 2^31 - 1")
    return m


def tail_select(fid, alpha: float, want=TAIL_SELECT_OUTPUTS, device=None):
    """The lower tail of every row of `fid` (C, K), selected on the GPU in one launch (`rc_tail_select_f64_async`): dict of

        "list"   (C, m) int32     m = min(K, ceil(alpha K)): the indices of the m smallest values of the row under the order
                                  (value, index) - ties to the lower index -, in ascending index order,
        "weight" (C, m) float64   1 / (alpha K), and (alpha K - (m - 1)) / (alpha K) on the m-th smallest element,
        "var"    (C,)   float64   the m-th smallest value (the value at risk),

    the entries named in `want` ("list" always): the bits of `noise.tail_weights` (NumPy route), which is the definition.  -0.0
    and +0.0 tie; a row with a NaN gives -1 / 0.0 / NaN.  A float64 torch CUDA tensor in: torch tensors on its device, enqueued on
    the current stream, no host synchronisation.  A NumPy array in: uploaded (to `device`), NumPy arrays out."""
    alpha = float(alpha)
    if not (0.0 < alpha <= 1.0):
        raise ValueError("alpha must be in (0, 1]")
    want = _check_want(want, TAIL_SELECT_OUTPUTS, allow_empty=True)
    if fid.ndim != 2:
        raise ValueError("fid: expected (C, K)")
    C, K = (int(v) for v in fid.shape)
    if K == 0:
        raise ValueError("fid: K must be positive")
    if K > 2 ** 31 - 1:
        raise ValueError("fid: K must be at most 2^31 - 1")
    lib = _lib.load()
    _lib.require_gpu()
    import torch
    host = not _is_torch(fid)
    if host:
        dev = compute_device() if device is None else torch.device("cuda", device_index(device))
        fid = torch.from_numpy(np.ascontiguousarray(fid, dtype=np.float64)).to(dev)
    fid = fid.contiguous()
    if not _is_dev_f64(fid):
        raise ValueError("fid must be a float64 CUDA tensor (or a NumPy array, which is uploaded)")
    dev = fid.device
    m = tail_select_len(K, alpha)
    res, out_ptr = _outputs(TAIL_SELECT_OUTPUTS, [k for k in TAIL_SELECT_OUTPUTS if k == "list" or k in want],
                            {"list": (C, m), "weight": (C, m), "var": (C,)}, dev, dtypes={"list": torch.int32})
    _lib.check(lib.rc_tail_select_f64_async(*_on_stream(dev), _dev_ptr(fid), C, K, alpha, *out_ptr))
    if host:
        return {k: v.cpu().numpy() for k, v in res.items()}
    return res


BOOTSTRAP_OUTPUTS = ("summary", "replicates")
BOOTSTRAP_ROUTES = {"auto": 0, "lds": 1, "global": 2}


def bootstrap_metrics(fid, n_boot: int, seed: int, offset: int = 0, q_thresholds=Q_THRESHOLDS, conf: float = 0.95,
                      want=BOOTSTRAP_OUTPUTS, route: str = "auto", device=None):
    """Bootstrap of the per-row metrics of `fid` (C, K), resampled on the GPU (`rc_bootstrap_metrics_f64_async`; the definition
    is `bootstrap.py`): `n_boot` resamples of every row with replacement from the counter-based stream (`seed`, `offset` in Philox
    counters; row c of a C-row call equals row 0 of a one-row call at offset + c n_boot ceil(K / 4)).  Dict of the entries named
    in `want`,

        "replicates" (M, C, B)   every metric of every replicate,
        "summary"    (M, 4, C)   per metric and row: mean, standard error (ddof = 1; NaN for n_boot = 1), and the lower and upper
                                 end of the two-sided percentile interval at level `conf` (`bootstrap.ranks`: NumPy's quantile
                                 methods "lower" and "higher"),

    plus "names": the M = 3 + nq metrics in order, rim1, std, min, q0 ... (signs of `reduce_metrics`: q and min positive).  A row
    with a NaN gives NaN.  `route`: "auto", "lds" (the row is staged in LDS; K <= 18 432) or "global"; the routes give the same
    bits.  A float64 torch CUDA tensor in: torch tensors on its device, enqueued on the current stream, no host synchronisation.
    A NumPy array in: NumPy arrays out (the blocking entry)."""
    from . import bootstrap as _boot
    want = _check_want(want, BOOTSTRAP_OUTPUTS)
    if route not in BOOTSTRAP_ROUTES:
        raise ValueError(f"route: one of {tuple(BOOTSTRAP_ROUTES)}, got {route!r}")
    if fid.ndim != 2:
        raise ValueError("fid: expected (C, K)")
    C, K = (int(v) for v in fid.shape)
    B = int(n_boot)
    if K < 1:
        raise ValueError("fid: K must be positive")
    if not 1 <= B <= _boot.MAX_N_BOOT:
        raise ValueError(f"n_boot must be in 1 .. {_boot.MAX_N_BOOT}")
    seed, offset = int(seed), int(offset)
    if not (0 <= seed < 2 ** 64 and 0 <= offset < 2 ** 64):
        raise ValueError("seed and offset must be in 0 .. 2^64 - 1")
    rank_lo, rank_hi = _boot.ranks(B, conf)
    thr = np.ascontiguousarray(q_thresholds, dtype=np.float64).reshape(-1)
    nq = int(thr.size)
    M = 3 + nq
    lib = _lib.load()
    _lib.require_gpu()
    order = ("replicates", "summary")                # (of the C entry's outputs, and of the dict)
    shapes = {"replicates": (M, C, B), "summary": (M, 4, C)}
    args = (C, K, B, seed, offset, _ptr(thr) if nq else None, nq, rank_lo, rank_hi, BOOTSTRAP_ROUTES[route])
    if _is_torch(fid):
        fid = fid.contiguous()
        if not _is_dev_f64(fid):
            raise ValueError("fid must be a float64 CUDA tensor (or a NumPy array)")
        res, out_ptr = _outputs(order, [k for k in order if k in want], shapes, fid.device)
        _lib.check(lib.rc_bootstrap_metrics_f64_async(*_on_stream(fid.device), _dev_ptr(fid), *args, *out_ptr))
    else:
        fid = np.ascontiguousarray(fid, dtype=np.float64)
        res, out_ptr = _outputs(order, [k for k in order if k in want], shapes)
        _lib.check(lib.rc_bootstrap_metrics_f64(device_index(device), _ptr(fid), *args, *out_ptr))
    res["names"] = _boot.metric_names(nq)
    return res


def _sorted_rows_on_device(lib, t):
    """The rows of the contiguous float64 CUDA tensor `t` (C, K) sorted ascending by the library's row sort, on the current stream."""
    import torch
    srt = torch.empty_like(t)
    C, K = (int(v) for v in t.shape)
    if C and K:
        _lib.check(lib.rc_reduce_ex_f64_async(*_on_stream(t.device), _dev_ptr(t), C, K, None, 0, 0.0, None, None, None, None,
                                              _dev_ptr(srt), 0))
    return srt


def sort_rows(fid, device=None):
    """The rows of `fid` (C, K) sorted ascending by the library's row sort (what `reduce_metrics(want_sorted=True)["sorted"]` holds,
    without the metrics): a float64 torch CUDA tensor in, a tensor out, on the current stream; a NumPy array in, an array out."""
    lib = _lib.load()
    _lib.require_gpu()
    if fid.ndim != 2:
        raise ValueError("fid: expected (C, K)")
    if _is_torch(fid):
        fid = fid.contiguous()
        if not _is_dev_f64(fid):
            raise ValueError("fid must be a float64 CUDA tensor (or a NumPy array)")
        return _sorted_rows_on_device(lib, fid)
    fid = np.ascontiguousarray(fid, dtype=np.float64)
    srt = np.empty_like(fid)
    if fid.size:
        _lib.check(lib.rc_reduce_f64(device_index(device), _ptr(fid), fid.shape[0], fid.shape[1], None, 0, 0.0, None, None, None, None,
                                     _ptr(srt)))
    return srt


def wasserstein_matrix(a, b=None, p: int = 1, assume_sorted: bool = False, device=None, out=None):
    """Pairwise p-Wasserstein distances between the rows of `a` (CA, K) and of `b` (CB, K) on the GPU
    (`rc_wasserstein_matrix_f64_async`; the definition is `wasserstein.matrix_reference`): out[i, j] = (mean_k |a_i(k) - b_j(k)|^p)^(1/p)
    over the SORTED rows, p = 1 or 2 - for equal-size samples the exact distance between the two empirical distributions.
    `b=None`: `a` against itself, (CA, CA), bit-for-bit symmetric with a zero diagonal.  A row holding a NaN gives NaN in its whole
    row and column.  The rows are sorted with the library's row sort unless `assume_sorted` says they already are (what
    `reduce_metrics(want_sorted=True)["sorted"]` holds).  An element's bits depend on its two rows, K and p alone.
    Float64 torch CUDA tensors in: a torch tensor on their device (`out`: a preallocated one to fill), enqueued on the current
    stream, no host synchronisation.  NumPy arrays in: a NumPy array out (the blocking entry on GPU `device`)."""
    p = int(p)
    if p not in (1, 2):
        raise ValueError("p must be 1 or 2")
    if a.ndim != 2 or (b is not None and (b.ndim != 2 or b.shape[1] != a.shape[1])):
        raise ValueError("a: expected (CA, K), b: (CB, K) with the same K")
    if b is not None and _is_torch(a) != _is_torch(b):
        raise ValueError("a and b: both NumPy arrays or both torch CUDA tensors")
    CA, K = (int(v) for v in a.shape)
    CB = int(b.shape[0]) if b is not None else 0
    shape = (CA, CB if b is not None else CA)
    lib = _lib.load()
    _lib.require_gpu()
    if _is_torch(a):
        import torch
        a = a.contiguous()
        b = None if b is None else b.contiguous()
        if not _is_dev_f64(a) or (b is not None and not (_is_dev_f64(b) and b.device == a.device)):
            raise ValueError("a and b must be float64 CUDA tensors on one device (or NumPy arrays)")
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=a.device)
        elif not (_is_dev_f64(out, shape) and out.device == a.device):
            raise ValueError(f"out: a contiguous float64 CUDA tensor of shape {shape} on the inputs' device")
        if not assume_sorted:
            a = _sorted_rows_on_device(lib, a)
            b = None if b is None else _sorted_rows_on_device(lib, b)
        _lib.check(lib.rc_wasserstein_matrix_f64_async(*_on_stream(a.device), p, _dev_ptr(a), CA, _dev_ptr(b), CB, K, _dev_ptr(out)))
        return out
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
    if out is None:
        out = np.empty(shape, dtype=np.float64)
    elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.shape == shape and out.flags.c_contiguous):
        raise ValueError(f"out: a C-contiguous float64 array of shape {shape}")
    _lib.check(lib.rc_wasserstein_matrix_f64(device_index(device), p, _ptr(a), CA, _ptr(b), CB, K, 1 if assume_sorted else 0, _ptr(out)))
    return out


LBFGS_KINDS = {"raw": 0, "one_minus": 1, "one_minus_plus_std": 2}
LBFGS_DEFAULTS = {"c1": 1e-4, "gtol": 1e-6, "ftol": 0.0, "maxiter": 100, "maxback": 20}


def _lbfgs_dims(ndim: int, m: int):
    ndim, m = int(ndim), int(m)
    if not 3 <= ndim <= 13:
        raise ValueError("ndim must be 3 .. 13 (N + 1, N = 2 .. max_nspin_grad())")
    if not 1 <= m <= 8:
        raise ValueError("m must be 1 .. 8")
    return ndim, m


def lbfgs_state_len(n_rows: int, ndim: int, m: int) -> int:
    """Doubles of batched L-BFGS state for `n_rows` rows of `ndim` variables with `m` pairs (`rc_lbfgs_state_len`, host only)."""
    ndim, m = _lbfgs_dims(ndim, m)
    if int(n_rows) < 0:
        raise ValueError("n_rows must be non-negative")
    n = int(_lib.load().rc_lbfgs_state_len(int(n_rows), ndim, m))
    if n < 0:
        raise ValueError("rc_lbfgs_state_len: bad arguments")
    return n


def _lbfgs_tensor(t, shape, what):
    if not _is_dev_f64(t, shape):
        raise ValueError(f"{what}: a contiguous float64 CUDA tensor of shape {tuple(shape)}")
    return t


def _lbfgs_bounds(bounds, like):
    """bounds = (lo, hi), tensors broadcastable to the (C, n) of `like` -> two contiguous float64 (C, n) tensors on its device (a
    tensor that already is one is passed through, so a caller who expands once hands in the same storage at every call)"""
    import torch
    if not (isinstance(bounds, (tuple, list)) and len(bounds) == 2 and all(_is_torch(b) for b in bounds)):
        raise ValueError("bounds: a pair (lo, hi) of torch tensors broadcastable to (C, n)")
    out = []
    for b, what in zip(bounds, ("lo", "hi")):
        if b.device != like.device:
            raise ValueError(f"bounds: {what} lives on another device than the rows")
        try:
            b = b.to(dtype=torch.float64).expand(tuple(like.shape)).contiguous()
        except RuntimeError:
            raise ValueError(f"bounds: {what} of shape {tuple(b.shape)} does not broadcast to {tuple(like.shape)}") from None
        out.append(b)
    return out


def lbfgs_init(x0, mask=None, m: int = 5, bounds=None):
    """Start the batched L-BFGS state machine (`rc_lbfgs_init_f64_async`; the definition is `lbfgs.py`): x0 (C, n) float64 CUDA
    tensor of start rows, `mask` (C, n) of 0 / 1 or None (a masked variable never moves) -> (state, trial): the opaque state
    (fields, C) and the (C, n) trial points - the `controllers` of the next gradient launch.  Enqueued on the current stream.
    `bounds` = (lo, hi), tensors broadcastable to (C, n) with -inf / +inf for a side without a bound: the BOXED machine
    (`rc_lbfgs_init_box_f64_async`) - the start rows are projected into the box, and every `lbfgs_advance` of this state must be
    given the same bounds."""
    if not _is_torch(x0) or x0.ndim != 2:
        raise ValueError("x0: a (C, n) float64 CUDA tensor")
    C, n = (int(v) for v in x0.shape)
    n, m = _lbfgs_dims(n, m)
    import torch
    x0 = _lbfgs_tensor(x0.contiguous() if x0.is_cuda and x0.dtype == torch.float64 else x0, (C, n), "x0")
    if mask is not None:
        mask = _lbfgs_tensor(mask, (C, n), "mask")
        if mask.device != x0.device:
            raise ValueError("mask lives on another device than x0")
    if bounds is not None:
        lo, hi = _lbfgs_bounds(bounds, x0)
    lib = _lib.load()
    _lib.require_gpu()
    dev = x0.device
    fields = 4 * n + 2 * m * n + m + 11
    if lbfgs_state_len(C, n, m) != fields * C:
        raise _lib.RobCharHipError("rc_lbfgs_state_len disagrees with the state layout of lbfgs.py")
    state = torch.empty((fields, C), dtype=torch.float64, device=dev)
    trial = torch.empty((C, n), dtype=torch.float64, device=dev)
    if bounds is not None:
        _lib.check(lib.rc_lbfgs_init_box_f64_async(*_on_stream(dev), n, m, C, _dev_ptr(x0), _dev_ptr(mask), _dev_ptr(lo), _dev_ptr(hi),
                                                   _dev_ptr(state), _dev_ptr(trial)))
    else:
        _lib.check(lib.rc_lbfgs_init_f64_async(*_on_stream(dev), n, m, C, _dev_ptr(x0), _dev_ptr(mask), _dev_ptr(state), _dev_ptr(trial)))
    return state, trial


def _lbfgs_state_dims(state, trial, m):
    if not (_is_torch(trial) and trial.ndim == 2):
        raise ValueError("trial: the (C, n) tensor of lbfgs_init")
    C, n = (int(v) for v in trial.shape)
    n, m = _lbfgs_dims(n, m)
    _lbfgs_tensor(trial, (C, n), "trial")
    _lbfgs_tensor(state, (4 * n + 2 * m * n + m + 11, C), "state")
    if state.device != trial.device:
        raise ValueError("state and trial live on different devices")
    return C, n, m


def lbfgs_advance(state, trial, row_a, row_b=None, *, m: int = 5, kind="one_minus", lam: float = 0.0, c1: float = 1e-4,
                  gtol: float = 1e-6, ftol: float = 0.0, maxiter: int = 100, maxback: int = 20, bounds=None):
    """One step of every row (`rc_lbfgs_advance_f64_async`; with `bounds` = the (lo, hi) given to `lbfgs_init`, the boxed
    `rc_lbfgs_advance_box_f64_async`: projected trial points, the active set, the projected-gradient test): `row_a` (C, n + 1) holds what a gradient entry wrote for the rows
    of `trial` - kind "raw": (f, g); "one_minus": a "mean" or "sum" row, f = 1 - a[0], g = -a[1:]; "one_minus_plus_std": `row_a`
    = "mean", `row_b` = "moment", f = 1 - mean F + lam std F.  Per row: accept or backtrack, and the next trial point written
    into `trial` in place (all NaN for a row that is done).  `m` as given to `lbfgs_init`.  Enqueue-only, current stream."""
    if kind not in LBFGS_KINDS:
        raise ValueError(f"kind: one of {tuple(LBFGS_KINDS)}")
    C, n, m = _lbfgs_state_dims(state, trial, m)
    _lbfgs_tensor(row_a, (C, n + 1), "row_a")
    if kind == "one_minus_plus_std":
        _lbfgs_tensor(row_b, (C, n + 1), "row_b")
    else:
        row_b = None
    if not (0.0 < float(c1) < 1.0) or not float(gtol) >= 0.0 or not float(ftol) >= 0.0 or int(maxiter) < 1 or int(maxback) < 0:
        raise ValueError("c1 in (0, 1), gtol >= 0, ftol >= 0, maxiter >= 1, maxback >= 0")
    if any(t is not None and t.device != state.device for t in (row_a, row_b)):
        raise ValueError("row_a / row_b live on another device than the state")
    if bounds is not None:
        lo, hi = _lbfgs_bounds(bounds, trial)
    lib = _lib.load()
    _lib.require_gpu()
    head = (*_on_stream(state.device), n, m, C, LBFGS_KINDS[kind], float(lam), _dev_ptr(row_a), _dev_ptr(row_b))
    tail = (float(c1), float(gtol), float(ftol), int(maxiter), int(maxback), _dev_ptr(state), _dev_ptr(trial))
    if bounds is not None:
        _lib.check(lib.rc_lbfgs_advance_box_f64_async(*head, _dev_ptr(lo), _dev_ptr(hi), *tail))
    else:
        _lib.check(lib.rc_lbfgs_advance_f64_async(*head, *tail))


LBFGS_RESULT_OUTPUTS = ("x", "f", "grad", "status", "iters", "evals")


def lbfgs_result(state, trial, *, m: int = 5, want=LBFGS_RESULT_OUTPUTS):
    """The rows' results out of the state (`rc_lbfgs_result_f64_async`): dict of torch tensors on the state's device, the entries
    named in `want`: "x" (C, n), "f" (C,), "grad" (C, n) float64, "status" (C,) int32 (0 running, 1 gtol, 2 ftol, 3 maxiter,
    4 line search failed, 5 not finite), "iters" and "evals" (C,) int64.  Enqueue-only, current stream."""
    want = _check_want(want, LBFGS_RESULT_OUTPUTS)
    C, n, m = _lbfgs_state_dims(state, trial, m)
    lib = _lib.load()
    _lib.require_gpu()
    import torch
    res, out_ptr = _outputs(LBFGS_RESULT_OUTPUTS, want, {"x": (C, n), "f": (C,), "grad": (C, n), "status": (C,), "iters": (C,), "evals": (C,)},
                            state.device, dtypes={"status": torch.int32, "iters": torch.int64, "evals": torch.int64})
    _lib.check(lib.rc_lbfgs_result_f64_async(*_on_stream(state.device), n, m, C, _dev_ptr(state), *out_ptr))
    return res


def mc_fidelity_directional(controllers, idx, ab, nspin: int, inspin: int, outspin: int, n_draws: int, h0_diag=None,
                            h0_offdiag=None, out=None):
    """Fidelities of `directional_perturbation` samples straight from (direction index, two normals) per sample
    (`rc_mc_fidelity_directional_f64_async`): controllers (C, N+1) torch CUDA tensor, idx (C*K,) int32, ab (C*K, 2) float64
    - what `directional_draws_device` returns - -> (C, K) torch tensor on the same device, enqueued on the current stream.
    Chain topology, N <= 12 (the library answers RC_ENOSUP otherwise: `RobCharHipError`)."""
    import torch
    _check_geometry(nspin, inspin, outspin)
    lib = _lib.load()
    _lib.require_gpu()
    if not (_is_torch(idx) and _is_torch(ab) and _is_torch(controllers)):
        raise ValueError("controllers, idx and ab must be torch tensors (idx / ab: what directional_draws_device returns)")
    dev = idx.device
    C, K = int(controllers.shape[0]), int(n_draws)
    if not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() == C * K):
        raise ValueError("idx must be a contiguous int32 CUDA tensor with C * K entries")
    if not (_is_dev_f64(ab, (C * K, 2)) and ab.device == dev):
        raise ValueError("ab must be a contiguous float64 CUDA tensor of shape (C * K, 2) on idx's device")
    if controllers.is_cuda and controllers.device != dev:
        raise ValueError("controllers live on another GPU than idx / ab")
    ctrl = _controllers_on(controllers, dev, C, nspin)
    if out is None:
        out = torch.empty((C, K), dtype=torch.float64, device=dev)
    elif not (_is_dev_f64(out, (C, K)) and out.device == dev):
        raise ValueError("out must be a contiguous float64 CUDA tensor of shape (C, K) on idx's device")
    h0d, h0o = _static_terms(h0_diag, h0_offdiag, nspin)
    _lib.check(lib.rc_mc_fidelity_directional_f64_async(*_on_stream(dev), nspin, inspin, outspin, _ptr(h0d), _ptr(h0o), 0,
                                                        _dev_ptr(ctrl), _dev_ptr(idx), _dev_ptr(ab), C, K, _dev_ptr(out)))
    return out


def mc_fidelity_nonhermitian(controllers, draws, diag_imag, nspin: int, inspin: int, outspin: int, h0_diag=None,
                             h0_offdiag=None, ring: bool = False, device=None):
    """Fidelities for a Hamiltonian with an IMAGINARY diagonal perturbation: H = HH + Z(draws) + diag(x) +
    1j*diag(diag_imag) - the dense Pade-expm kernel (`rc_mc_fidelity_nh_f64_async`).  controllers (C, N+1), draws
    (C, K, N, 3), diag_imag (C, K, N) or None -> (C, K).  NumPy in / NumPy out, torch CUDA in / torch out."""
    _check_geometry(nspin, inspin, outspin)
    lib = _lib.load()
    _lib.require_gpu()
    import torch
    as_numpy = not _is_torch(draws)
    dev = torch.device("cuda", device_index(device)) if as_numpy else draws.device
    to_dev = lambda a: None if a is None else (a if _is_torch(a) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))).to(device=dev, dtype=torch.float64).contiguous()
    d, c, g = to_dev(draws), to_dev(controllers), to_dev(diag_imag)
    C, K = int(d.shape[0]), int(d.shape[1])
    if tuple(d.shape) != (C, K, nspin, 3) or tuple(c.shape) != (C, nspin + 1) or (g is not None and tuple(g.shape) != (C, K, nspin)):
        raise ValueError("shapes: controllers (C, N+1), draws (C, K, N, 3), diag_imag (C, K, N)")
    out = torch.empty((C, K), dtype=torch.float64, device=dev)
    h0d, h0o = _static_terms(h0_diag, h0_offdiag, nspin)
    _lib.check(lib.rc_mc_fidelity_nh_f64_async(*_on_stream(dev), nspin, inspin, outspin, _ptr(h0d), _ptr(h0o), int(bool(ring)),
                                               _dev_ptr(c), _dev_ptr(d), _dev_ptr(g), C, K, _dev_ptr(out)))
    return out.cpu().numpy() if as_numpy else out


def release_stream(stream=None, device=None) -> None:
    """Hand back what the library keeps for `stream` (a torch.cuda.Stream; default: the current one) - the repair list of
    the ring-topology route, 10 bytes per sample of the largest ring launch the stream ran (`rc_release_stream`; freed in
    stream order behind the stream's last launch).  Call it before retiring a side stream that ran ring launches; the
    library also caps what unreleased streams can hold (16 buffers per device, least recently used evicted)."""
    import torch
    lib = _lib.load()
    _lib.require_gpu()
    if stream is None:
        stream = torch.cuda.current_stream(torch.device("cuda", device_index(device)))
    _lib.check(lib.rc_release_stream(int(stream.device.index or 0), ctypes.c_void_p(stream.cuda_stream)))


class ring_stream:
    """Context manager: a side stream for ring-topology launches whose library-side buffer is released on exit.

        with backend.ring_stream(device) as st:            # torch.cuda.Stream, current inside the block
            backend.mc_fidelity(ctrl, draws, N, a, b, ring=True, out=fid)
    """

    def __init__(self, device=None, priority: int = 0):
        import torch
        self._torch = torch
        self.stream = torch.cuda.Stream(torch.device("cuda", device_index(device)), priority=priority)
        self._ctx = None

    def __enter__(self):
        self._ctx = self._torch.cuda.stream(self.stream)
        self._ctx.__enter__()
        return self.stream

    def __exit__(self, *exc):
        try:
            release_stream(self.stream)
        finally:
            self._ctx.__exit__(*exc)
        return False


def general_path_tiles(device=None, reset: bool = False) -> int:
    """Diagnostic: 64-sample tiles that left the chain kernels' fast path since the last reset (0 on healthy
    workloads; each such tile is recomputed by the much slower general per-sample routine)."""
    _lib.require_gpu()
    return _tile_counter("rc_stats_general_tiles", device, reset)


def polish_tiles(device=None, reset: bool = False) -> int:
    """Diagnostic: 64-sample tiles of the mixed-precision eigenvalue path that needed more than its one fp64 step since
    the last reset (a close eigenvalue pair somewhere in the tile; the tile keeps stepping, still on the fast path)."""
    _lib.require_gpu()
    return _tile_counter("rc_stats_polish_tiles", device, reset)


def _devices_arg(devices):
    if devices is None:
        n = _lib.require_gpu()
        devices = list(range(n))
    devices = [int(d) for d in devices]
    return (ctypes.c_int * len(devices))(*devices), len(devices)


def mc_fidelity_sharded(controllers, draws, nspin: int, inspin: int, outspin: int, devices=None, h0_diag=None,
                        h0_offdiag=None, ring: bool = False, kernel: str = "auto"):
    """`mc_fidelity` over several GPUs of this process (`rc_mc_fidelity_sharded_f64`): host arrays in, the full
    (C, K) host array out; controllers are split into contiguous blocks, one per device."""
    _check_geometry(nspin, inspin, outspin)
    lib = _lib.load()
    dev_arr, ndev = _devices_arg(devices)
    draws = np.ascontiguousarray(draws, dtype=np.float64)
    if draws.ndim != 4 or draws.shape[2:] != (nspin, 3):
        raise ValueError(f"draws: expected (C, K, {nspin}, 3), got {draws.shape}")
    C, K = draws.shape[:2]
    ctrl = _np_f64(controllers, (C, nspin + 1), "controllers")
    res = np.empty((C, K))
    h0d, h0o = _static_terms(h0_diag, h0_offdiag, nspin)
    _lib.check(lib.rc_mc_fidelity_sharded_f64(ndev, dev_arr, _lib.KERNELS[kernel], nspin, inspin, outspin,
                                              _ptr(h0d), _ptr(h0o), int(bool(ring)), _ptr(ctrl), _ptr(draws), C, K, _ptr(res)))
    return res


def mc_metrics_sharded(controllers, n_draws: int, nspin: int, inspin: int, outspin: int, draws=None, seed: int = 0,
                       offset: int = 0, sigma: float = 0.0, devices=None, h0_diag=None, h0_offdiag=None,
                       ring: bool = False, kernel: str = "auto", q_thresholds=Q_THRESHOLDS, dkw_eps: float = 0.0,
                       want_fid: bool = False):
    """Fidelity + per-controller metrics over several GPUs of this process (`rc_mc_metrics_sharded_f64`); only the
    metric rows (and the fidelities when `want_fid`) come back to the host.  `draws=None`: counter-based draws
    generated on the devices (stream `seed`, first element `offset`, scaled by `sigma`)."""
    _check_geometry(nspin, inspin, outspin)
    lib = _lib.load()
    dev_arr, ndev = _devices_arg(devices)
    ctrl = np.ascontiguousarray(controllers, dtype=np.float64)
    C, K = ctrl.shape[0], int(n_draws)
    if ctrl.shape != (C, nspin + 1):
        raise ValueError(f"controllers: expected (C, {nspin + 1})")
    if draws is not None:
        draws = _np_f64(draws, (C, K, nspin, 3), "draws")
    thr = np.ascontiguousarray(q_thresholds, dtype=np.float64)
    nq = int(thr.size)
    res = {"rim1": np.empty((3, C)), "std": np.empty((3, C)), "min": np.empty((3, C)), "q": np.empty((3, nq, C))}
    fid = np.empty((C, K)) if want_fid else None
    h0d, h0o = _static_terms(h0_diag, h0_offdiag, nspin)
    _lib.check(lib.rc_mc_metrics_sharded_f64(ndev, dev_arr, _lib.KERNELS[kernel], nspin, inspin, outspin,
                                             _ptr(h0d), _ptr(h0o), int(bool(ring)), _ptr(ctrl), _ptr(draws), int(seed), int(offset), float(sigma), C, K,
                                             _ptr(thr), nq, float(dkw_eps), _ptr(res["rim1"]), _ptr(res["std"]),
                                             _ptr(res["min"]), _ptr(res["q"]) if nq else None, _ptr(fid)))
    if want_fid:
        res["fid"] = fid
    return res


class RcclComm:
    """`rc_comm_init` / `rc_comm_destroy` as a context manager: ONE process, one RCCL communicator per listed GPU - the
    exchange step of the path (an all-gather over xGMI) from the C ABI, without torch.distributed.

        with backend.RcclComm(devices=[0, 1, 2, 3]) as comm:
            res = backend.mc_metrics_gathered(comm, controllers, K, N, a, b, seed=7, sigma=0.05)
    """

    def __init__(self, devices=None):
        # PyTorch first: the library resolves RCCL from what the process already carries (torch ships its own librccl.so /
        # librocm_smi64.so) and only otherwise opens the system's; a process that ends up with BOTH pairs is one ROCm
        # does not expect (robchar_hip.hip: rccl_api)
        import torch  # noqa: F401
        self.lib = _lib.load()
        dev_arr, ndev = _devices_arg(devices)
        self.devices = [int(d) for d in dev_arr]           # rank r of the communicator = GPU devices[r]
        self.handle = ctypes.c_void_p()
        _lib.check(self.lib.rc_comm_init(ndev, dev_arr, ctypes.byref(self.handle)))
        self.ndev = int(self.lib.rc_comm_size(self.handle))

    def close(self):
        if self.handle:
            _lib.check(self.lib.rc_comm_destroy(self.handle))
            self.handle = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def mc_metrics_gathered(comm: "RcclComm", controllers, n_draws: int, nspin: int, inspin: int, outspin: int, draws=None,
                        seed: int = 0, offset: int = 0, sigma: float = 0.0, h0_diag=None, h0_offdiag=None, ring: bool = False,
                        kernel: str = "auto", q_thresholds=Q_THRESHOLDS, dkw_eps: float = 0.0, want_fid: bool = False):
    """Fidelity + per-controller metrics over the communicator's GPUs with the exchange step ON the devices
    (`rc_mc_metrics_gathered_f64`: every device all-gathers the metric rows - and the fidelity slabs when `want_fid` - over
    RCCL); returns the host copies (from the first device) in `mc_metrics_sharded`'s format.  The device-resident gathered
    buffers are the library's own here (a C caller can pass its own and keep them)."""
    _check_geometry(nspin, inspin, outspin)
    lib = _lib.load()
    ctrl = np.ascontiguousarray(controllers, dtype=np.float64)
    C, K = ctrl.shape[0], int(n_draws)
    if ctrl.shape != (C, nspin + 1):
        raise ValueError(f"controllers: expected (C, {nspin + 1})")
    if draws is not None:
        draws = _np_f64(draws, (C, K, nspin, 3), "draws")
    thr = np.ascontiguousarray(q_thresholds, dtype=np.float64)
    nq = int(thr.size)
    table = np.empty((9 + 3 * nq, C))
    fid = np.empty((C, K)) if want_fid else None
    fid_dev = None
    keep = []
    if want_fid and comm.ndev > 1:                    # a fidelity gather needs a receive buffer on every rank
        import torch
        cmax = -(-C // comm.ndev)
        for d in comm.devices:                        # rank r's receive buffer lives on GPU devices[r]
            keep.append(torch.empty((comm.ndev * cmax * K,), dtype=torch.float64, device=torch.device("cuda", d)))
        fid_dev = (ctypes.c_void_p * comm.ndev)(*[_dev_ptr(t) for t in keep])
    h0d, h0o = _static_terms(h0_diag, h0_offdiag, nspin)
    _lib.check(lib.rc_mc_metrics_gathered_f64(comm.handle, _lib.KERNELS[kernel], nspin, inspin, outspin,
                                              _ptr(h0d), _ptr(h0o), int(bool(ring)), _ptr(ctrl), _ptr(draws), int(seed), int(offset), float(sigma), C, K,
                                              _ptr(thr), nq, float(dkw_eps), None, fid_dev, _ptr(table), _ptr(fid)))
    res = {"rim1": table[0:3].copy(), "std": table[3:6].copy(), "min": table[6:9].copy(),
           "q": table[9:].reshape(3, nq, C).copy()}
    if want_fid:
        res["fid"] = fid
    return res


# ---- randomised quasi-Monte Carlo: scrambled Sobol points (the definition: sobol.py) --------------------------------------------
MAX_NSPIN_SOBOL = 13                 # RC_MAX_NSPIN_SOBOL of include/robchar_hip.h


def _sobol_tables(dirnum, shift, P, K, skip, C, D=None):
    """The Sobol arguments validated BEFORE the library is loaded -> (dirnum, shift, C, R, D, shift_cstride): dirnum (R, D, 32) (or
    (D, 32): one replicate), shift (Cs, R, D) with Cs = 1 (row 0 for every controller row, stride 0) or Cs = C (stride R D); the
    words as NumPy uint32 arrays or torch CUDA tensors of a 32-bit integer type (uint32 / int32: the bit patterns)."""
    from . import sobol
    if not _is_torch(dirnum):
        dirnum = np.ascontiguousarray(dirnum, dtype=np.uint32)
    if not _is_torch(shift):
        shift = np.ascontiguousarray(shift, dtype=np.uint32)
    if dirnum.ndim == 2:
        dirnum = dirnum[None]
    if dirnum.ndim != 3 or dirnum.shape[2] != 32:
        raise ValueError(f"dirnum: expected (R, D, 32), got {tuple(dirnum.shape)}")
    R, Dn = int(dirnum.shape[0]), int(dirnum.shape[1])
    if D is not None and Dn != D:
        raise ValueError(f"dirnum: expected {D} dimensions, got {Dn}")
    if shift.ndim == 2:
        shift = shift[None]
    if shift.ndim != 3 or tuple(shift.shape[1:]) != (R, Dn):
        raise ValueError(f"shift: expected (1 or C, {R}, {Dn}), got {tuple(shift.shape)}")
    Cs = int(shift.shape[0])
    C = Cs if C is None else int(C)
    if C < 0 or Cs not in (1, C):
        raise ValueError(f"shift: expected 1 or {C} rows, got {Cs}")
    sobol.check_contract(Dn, R, P, skip, K)
    return dirnum, shift, C, R, Dn, (R * Dn if (Cs == C and C > 1) else 0)


def _u32_on(t, dev):
    """Sobol words as a contiguous 32-bit integer tensor on `dev` (a NumPy uint32 array is uploaded)."""
    import torch
    if not _is_torch(t):
        return torch.from_numpy(t.view(np.int32)).to(dev)
    if t.element_size() != 4 or t.is_floating_point() or not t.is_cuda or not t.is_contiguous():
        raise ValueError("Sobol tables: contiguous CUDA tensors of a 32-bit integer type")
    return t


def _sobol_generate(want, dirnum, shift, P, K, skip, sigma, C, device, as_torch):
    dirnum, shift, C, R, D, stride = _sobol_tables(dirnum, shift, P, K, skip, C)
    K, P, skip = int(K), int(P), int(skip)
    per_row = not isinstance(sigma, (int, float)) and np.ndim(sigma) > 0
    if per_row and not _is_torch(sigma):
        sigma = np.ascontiguousarray(sigma, dtype=np.float64)
    if per_row and tuple(sigma.shape) != (C,):
        raise ValueError("sigma: a float or a (C,) tensor")
    lib = _lib.load()
    _lib.require_gpu()
    on_device = as_torch or _is_torch(dirnum) or _is_torch(shift)
    if on_device:
        import torch
        dev = next((t.device for t in (dirnum, shift) if _is_torch(t)), None)
        if dev is None:
            dev = device if hasattr(device, "type") else torch.device("cuda", device_index(device))
        dn, sh = _u32_on(dirnum, dev), _u32_on(shift, dev)
        rows = None
        if per_row:
            rows = (sigma if _is_torch(sigma) else torch.from_numpy(np.ascontiguousarray(sigma, dtype=np.float64))).to(
                device=dev, dtype=torch.float64).contiguous()
        res, out_ptr = _outputs(("draws", "bits"), want, {"draws": (C, K, D), "bits": (C, K, D)}, dev, {"bits": torch.int32})
        _lib.check(lib.rc_draws_sobol_f64_async(*_on_stream(dev), D, _dev_ptr(dn), _dev_ptr(sh), stride, R, P, skip,
                                                0.0 if per_row else float(sigma), _dev_ptr(rows), C, K, *out_ptr))
        return res
    rows = np.ascontiguousarray(sigma, dtype=np.float64) if per_row else None
    res = {k: np.empty((C, K, D), dtype=np.float64 if k == "draws" else np.uint32) for k in want}
    _lib.check(lib.rc_draws_sobol_f64(device_index(device), D, _ptr(dirnum), _ptr(shift), stride, R, P, skip,
                                      0.0 if per_row else float(sigma), _ptr(rows), C, K, _ptr(res.get("draws")), _ptr(res.get("bits"))))
    return res


def sobol_points(dirnum, shift, P: int, K: int, skip: int = 0, C=None, device=None, as_torch: bool = False):
    """The scrambled Sobol points of `sobol.points(dirnum, shift, P, K, skip, C)` made on the GPU (`rc_draws_sobol_f64[_async]`),
    bit for bit: (C, K, D) words.  NumPy tables in -> NumPy uint32 out (blocking); torch CUDA tables, or `as_torch` -> an int32
    torch tensor holding the words' bit patterns, enqueued on the current stream."""
    return _sobol_generate(("bits",), dirnum, shift, P, K, skip, 1.0, C, device, as_torch)["bits"]


def sobol_normal(dirnum, shift, P: int, K: int, skip: int = 0, sigma=1.0, C=None, device=None, as_torch: bool = False):
    """sigma-scaled normals of the scrambled Sobol points (`sobol.normals`, to a few ulp): (C, K, D) float64 - for D = 3 N,
    reshaped to (C, K, N, 3), the draw tensor every entry that reads draws takes.  Sample k of row c is point skip + (k mod P) of
    replicate k // P.  `sigma`: a float, or a (C,) array / tensor (one scale per controller row).  NumPy / torch as `sobol_points`."""
    return _sobol_generate(("draws",), dirnum, shift, P, K, skip, sigma, C, device, as_torch)["draws"]


def sobol_fused_supported(nspin: int, ring: bool = False, kernel: str = "auto") -> bool:
    """Can `mc_fidelity_sobol` take this geometry (chain, N <= 13, eigenvalue-only kernels)?"""
    return (not ring) and 2 <= nspin <= MAX_NSPIN_SOBOL and kernel in ("auto", "tridiag_adj")


def mc_fidelity_sobol(controllers, n_draws: int, nspin: int, inspin: int, outspin: int, dirnum, shift, P: int, skip: int = 0,
                      sigma=0.05, h0_diag=None, h0_offdiag=None, kernel: str = "auto", out=None):
    """Fidelities with the scrambled Sobol normals generated INSIDE the kernel (`rc_mc_fidelity_sobol_f64_async`): controllers
    (C, N+1) torch CUDA tensor (a NumPy array is uploaded to the current device) -> (C, K) torch tensor on that device, enqueued on
    the current stream; bit-identical to `mc_fidelity(controllers, sobol_normal(dirnum, shift, P, K, skip, sigma, C).view(C, K, N, 3))`
    without that tensor.  dirnum (R, 3 N, 32), shift (1 or C, R, 3 N): `sobol.scramble`; `sigma`: a float, or a (C,) tensor / array.
    Chain topology, N <= 13, kernel "auto" / "tridiag_adj"."""
    import torch
    _check_geometry(nspin, inspin, outspin)
    h0d, h0o = _static_terms(h0_diag, h0_offdiag, nspin)
    nrows = int(controllers.shape[0]) if hasattr(controllers, "shape") else len(controllers)
    dirnum, shift, C, R, D, stride = _sobol_tables(dirnum, shift, P, n_draws, skip, nrows, D=3 * nspin)
    ctrl, rows, C, K, draw_args = _generated_draws_args(controllers, n_draws, sigma, 0, 0, nspin)
    lib = _lib.load()
    dev = ctrl.device
    dn, sh = _u32_on(dirnum, dev), _u32_on(shift, dev)
    if out is None:
        out = torch.empty((C, K), dtype=torch.float64, device=dev)
    elif not _is_dev_f64(out, (C, K)):
        raise ValueError("out must be a contiguous float64 CUDA tensor of shape (C, K)")
    _lib.check(lib.rc_mc_fidelity_sobol_f64_async(*_on_stream(dev), _lib.KERNELS[kernel], nspin, inspin, outspin, _ptr(h0d), _ptr(h0o),
                                                  _dev_ptr(ctrl), _dev_ptr(dn), _dev_ptr(sh), stride, R, int(P), int(skip),
                                                  draw_args[2], draw_args[3], C, K, _dev_ptr(out)))
    return out


# ---- variance indices (ABI 20): the pick-freeze kernel; variance_indices.py is the definition ------------------------------------
PICKFREEZE_OUTPUTS = ("fid", "mean")
MAX_NSPIN_PICKFREEZE = 13            # RC_MAX_NSPIN_PICKFREEZE


def pickfreeze_supported(nspin: int, ring: bool = False, kernel: str = "auto") -> bool:
    """Can `mc_fidelity_pickfreeze_philox` take this geometry (chain, N <= 13, eigenvalue-only kernels)?"""
    return (not ring) and 2 <= nspin <= MAX_NSPIN_PICKFREEZE and kernel in ("auto", "tridiag_adj")


def mc_fidelity_pickfreeze_philox(controllers, n_draws: int, nspin: int, inspin: int, outspin: int, seed: int, groups,
                                  offset: int = 0, offset_b=None, sigma=0.05, h0_diag=None, h0_offdiag=None, want=("mean",),
                                  kernel: str = "auto"):
    """The pick-freeze evaluations behind the variance indices in ONE launch (`rc_mc_fidelity_pickfreeze_philox_f64_async`;
    `variance_indices` is the definition): per sample two draw vectors a (stream block at `offset`: the draws of
    `mc_fidelity_philox`) and b (at `offset_b`; None = the block behind a's, offset + C K 3N) are generated inside the kernel and
    the fidelity is evaluated on a, on b and on the G hybrids "b where `groups[g]` has the coordinate's bit, a elsewhere".
    controllers (C, N+1) torch CUDA tensor (a NumPy array is uploaded to the current device) -> dict of torch tensors on that
    device, the entries named in `want`, enqueued on the current stream:

        "fid"  (G + 2, C, K)   slab 0 = F(a), 1 = F(b), 2 + g = F(h_g): bit-identical to `mc_fidelity_philox` at the two offsets and
                               to `mc_fidelity` on `torch.where(mask_g, B, A)` of the two `philox_normal` tensors,
        "mean" (C, 3 + 2 G)    the means over k of F(a), F(b), D = (F(a) - F(b))^2 and per group T_g = (F(a) - F(h_g))^2,
                               U_g = (F(b) - F(h_g))^2  (`variance_indices.indices_from_means`: var = D / 2, total_g = T_g / D,
                               first_g = 1 - U_g / D); the same bits with or without "fid".

    `groups`: at most 64 uint64 masks over the coordinates 3 i + s (`variance_indices.kind_groups` ...); `sigma`: a float, or a
    (C,) tensor / array.  Chain topology, N <= 13, kernel "auto" / "tridiag_adj".  Everything is validated before the device is
    touched."""
    from . import variance_indices as vi
    _check_geometry(nspin, inspin, outspin)
    want = _check_want(want, PICKFREEZE_OUTPUTS)
    if kernel not in _lib.KERNELS:
        raise ValueError(f"kernel: one of {tuple(_lib.KERNELS)}")
    if not pickfreeze_supported(nspin, False, kernel):
        raise NotImplementedError("the pick-freeze kernel takes chains of N <= 13 spins and the kernels \"auto\" / \"tridiag_adj\" "
                                  "(otherwise: variance_indices on mc_fidelity outputs of the hybrid tensors)")
    masks = vi.check_groups(groups, nspin)
    G = int(masks.shape[0])
    h0d, h0o = _static_terms(h0_diag, h0_offdiag, nspin)
    nrows = int(controllers.shape[0]) if hasattr(controllers, "shape") else len(controllers)
    offset = int(offset) % 2 ** 64
    offset_b = vi.default_offset_b(offset, nrows, n_draws, nspin) if offset_b is None else int(offset_b) % 2 ** 64
    if int(n_draws) >= 0 and not vi.ranges_disjoint(offset, offset_b, nrows * int(n_draws) * 3 * nspin):
        raise ValueError("offset_b: the element ranges of offset and offset_b overlap (each covers C K 3N elements)")
    ctrl, rows, C, K, draw_args = _generated_draws_args(controllers, n_draws, sigma, seed, offset, nspin)
    lib = _lib.load()
    dev = ctrl.device
    res, out_ptr = _outputs(PICKFREEZE_OUTPUTS, want, {"fid": (G + 2, C, K), "mean": (C, 3 + 2 * G)}, dev)
    _lib.check(lib.rc_mc_fidelity_pickfreeze_philox_f64_async(
        *_on_stream(dev), _lib.KERNELS[kernel], nspin, inspin, outspin, _ptr(h0d), _ptr(h0o), _dev_ptr(ctrl), draw_args[0], draw_args[1],
        offset_b, draw_args[2], draw_args[3], _ptr(masks) if G else None, G, C, K, *out_ptr))
    return res
