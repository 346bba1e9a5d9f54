// lbfgs_init[_box]_kernel, lbfgs_advance[_box]_kernel<NDIM>, lbfgs_result_kernel: the batched L-BFGS state machine on the device
// (rc_lbfgs_init[_box]_f64_async / rc_lbfgs_advance[_box]_f64_async / rc_lbfgs_result_f64_async; the definition is lbfgs.py).
//
// Part of ONE translation unit: this file is #included by robchar_hip.hip INSIDE its anonymous namespace; it is not a stand-alone
// header.  The arithmetic of a row is lbfgs_core.h, which the host test compiles too.
//
// ONE LANE PER CONTROLLER ROW, 64 rows per wave and workgroup: with n <= 13 variables and m <= 8 pairs a row's step is a few
// hundred DEPENDENT fp64 operations - a wave per row would add shuffles and a second summation order and save nothing.  The state
// is the caller's buffer, laid out [field][C]: the lanes of a wave read and write 64 consecutive doubles.  The iterate, the
// gradient, the direction and the recursion's q are registers (NDIM is a template argument, every loop over it unrolled); the ring
// of pairs stays in global memory and is read at the run-time slot; the recursion's loops over the pairs are unrolled to the
// largest m with a per-lane predicate, so no per-lane array is indexed at run time.  Rows are in different phases of the search in
// the same wave: every branch is per lane, and there is no LDS, no atomic and no barrier.  Lanes beyond C return at once.
//
// lbfgs_init_box_kernel and lbfgs_advance_box_kernel<NDIM> are the boxed variant (ABI 14; advance_row_t<NDIM, true>): the bounds
// lo, hi are [C][ndim] rows like x0, read by a running row into registers; the projection and the active set are registers with
// compile-time indices.  They are kernels of their own, with their own argument block, so that the unbounded kernels keep their
// names, their kernel arguments and their code.
struct LbfgsAdvanceParams {
    double* state;          // [fields][C]
    double* trial;          // [C][ndim]
    const double* a;        // [C][ndim + 1]
    const double* b;        // [C][ndim + 1], kind 2 only
    long long C;
    int m, kind;
    double lam;
    rclb::Params opt;
};

__global__ __launch_bounds__(64) void lbfgs_init_kernel(double* state, double* trial, const double* x0, const double* mask, long long C,
                                                        int ndim, int m) {
    const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const rclb::Layout L{ndim, m};
    const rclb::StridedRow row{state, trial, C, c, ndim};
    rclb::init_row(row, L, x0 + c * ndim, mask ? mask + c * ndim : nullptr);
}

__global__ __launch_bounds__(64) void lbfgs_init_box_kernel(double* state, double* trial, const double* x0, const double* mask,
                                                            const double* lo, const double* hi, long long C, int ndim, int m) {
    const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const rclb::Layout L{ndim, m};
    const rclb::StridedRow row{state, trial, C, c, ndim};
    rclb::init_row_box(row, L, x0 + c * ndim, mask ? mask + c * ndim : nullptr, lo + c * ndim, hi + c * ndim);
}

template <int NDIM>
__global__ __launch_bounds__(64) void lbfgs_advance_kernel(const LbfgsAdvanceParams p) {
    const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
    if (c >= p.C) return;
    const rclb::Layout L{NDIM, p.m};
    const rclb::StridedRow row{p.state, p.trial, p.C, c, NDIM};
    double ft, gt[NDIM];
    rclb::objective<NDIM>(p.kind, p.lam, p.a + c * (NDIM + 1), p.kind == rclb::kOneMinusPlusStd ? p.b + c * (NDIM + 1) : nullptr, ft, gt);
    rclb::advance_row<NDIM>(row, L, p.opt, ft, gt);
}

struct LbfgsAdvanceBoxParams {
    LbfgsAdvanceParams adv;
    const double* lo;       // [C][ndim]
    const double* hi;       // [C][ndim]
};

template <int NDIM>
__global__ __launch_bounds__(64) void lbfgs_advance_box_kernel(const LbfgsAdvanceBoxParams q) {
    const LbfgsAdvanceParams& p = q.adv;
    const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
    if (c >= p.C) return;
    const rclb::Layout L{NDIM, p.m};
    const rclb::StridedRow row{p.state, p.trial, p.C, c, NDIM};
    double ft, gt[NDIM];
    rclb::objective<NDIM>(p.kind, p.lam, p.a + c * (NDIM + 1), p.kind == rclb::kOneMinusPlusStd ? p.b + c * (NDIM + 1) : nullptr, ft, gt);
    rclb::advance_row_box<NDIM>(row, L, p.opt, ft, gt, q.lo + c * NDIM, q.hi + c * NDIM);
}

// the result of every row out of the field-major state, in the row-major layout of the other entries; every output optional
__global__ __launch_bounds__(64) void lbfgs_result_kernel(const double* state, long long C, int ndim, int m, double* x, double* f,
                                                          double* g, int* status, long long* iters, long long* evals) {
    const long long c = (long long)blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const rclb::Layout L{ndim, m};
    auto ld = [&](int field) { return state[(long long)field * C + c]; };
    for (int i = 0; i < ndim; ++i) {
        if (x) x[c * ndim + i] = ld(L.x() + i);
        if (g) g[c * ndim + i] = ld(L.g() + i);
    }
    if (f) f[c] = ld(L.f());
    if (status) status[c] = (int)ld(L.status());
    if (iters) iters[c] = (long long)ld(L.iters());
    if (evals) evals[c] = (long long)ld(L.evals());
}
