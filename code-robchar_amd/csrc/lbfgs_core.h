// One row of the batched L-BFGS state machine (lbfgs_init_kernel / lbfgs_advance_kernel, k_lbfgs.inc.h) - plain C++ so that
// the CPU unit test runs the exact text of the kernel's step (tests/host/host_lbfgs.cpp); the product only ever runs it inside
// the kernels.  The definition is code-robchar_amd/lbfgs.py: this file restates it operation for operation - every dot product
// accumulated sequentially over the variable index from 0.0, every product rounded once before it is added, IEEE division and
// square root.
//
// The state of C rows is ONE buffer of Layout::fields() x C doubles, field-major ([field][C]): the lanes of a wave hold
// consecutive rows, so every access is 64 consecutive doubles.  Integers (count, head, nback, iters, evals, status, first) are
// stored as doubles.  The step is written against a row accessor (ld / st on a field, trial_ld / trial_st on the row of the
// (C, n) trial array); StridedRow is the one the kernels and the host test use.
//
// Two variants of the machine share this text: the unbounded one (advance_row, init_row) and the BOXED one (advance_row_box,
// init_row_box: box bounds lo <= x <= hi, projected steps - the rules are in lbfgs.py).  The step is advance_row_t<NDIM, BOX>;
// everything boxed sits behind `if constexpr (BOX)`, so the unbounded instantiation is the code it was before the box existed.
// The bounds are not state: lo and hi are the row's [n] bounds, handed in at every call.
#pragma once

#ifndef RC_HD
#if defined(__HIPCC__)
#define RC_HD __host__ __device__ __forceinline__
#else
#define RC_HD inline
#endif
#endif

// products must not be contracted into the addition that consumes them (hipcc contracts by default); g++ builds of the host
// test pass -ffp-contract=off
// (both pragmas are clang's: g++ -Wall -Werror, which builds the host test, must not see them)
#if defined(__clang__)
#define RCLB_NO_CONTRACT _Pragma("clang fp contract(off)")
#define RCLB_UNROLL _Pragma("unroll")
#else
#define RCLB_NO_CONTRACT
#define RCLB_UNROLL
#endif

namespace rclb {

constexpr int kMinDim = 3, kMaxDim = 13, kMaxM = 8;
constexpr int kRaw = 0, kOneMinus = 1, kOneMinusPlusStd = 2;          // objective kinds
constexpr double kPairEps = 1e-10;                                    // a pair is stored when sy > 0 and sy >= eps sqrt(ss) sqrt(yy)
constexpr double kVarFloor = 64.0 * 2.220446049250313e-16;            // 64 * 2^-52: noise.moments_from_sums

struct Params {
    double c1, gtol, ftol;
    long long maxiter, maxback;
};

// first field row of every field (lbfgs.field_offsets)
struct Layout {
    int n, m;
    RC_HD int x() const { return 0; }
    RC_HD int f() const { return n; }
    RC_HD int g() const { return n + 1; }
    RC_HD int d() const { return 2 * n + 1; }
    RC_HD int t() const { return 3 * n + 1; }
    RC_HD int gd() const { return 3 * n + 2; }
    RC_HD int S() const { return 3 * n + 3; }
    RC_HD int Y() const { return 3 * n + 3 + m * n; }
    RC_HD int sy() const { return 3 * n + 3 + 2 * m * n; }
    RC_HD int count() const { return sy() + m; }
    RC_HD int head() const { return sy() + m + 1; }
    RC_HD int nback() const { return sy() + m + 2; }
    RC_HD int iters() const { return sy() + m + 3; }
    RC_HD int evals() const { return sy() + m + 4; }
    RC_HD int fprev() const { return sy() + m + 5; }
    RC_HD int status() const { return sy() + m + 6; }
    RC_HD int first() const { return sy() + m + 7; }
    RC_HD int mask() const { return sy() + m + 8; }
    RC_HD int fields() const { return 4 * n + 2 * m * n + m + 11; }
};

struct StridedRow {
    double* state;      // [fields][C]
    double* trial;      // [C][n]
    long long C, c;
    int n;
    RC_HD double ld(int field) const { return state[(long long)field * C + c]; }
    RC_HD void st(int field, double v) const { state[(long long)field * C + c] = v; }
    RC_HD double trial_ld(int i) const { return trial[c * n + i]; }
    RC_HD void trial_st(int i, double v) const { trial[c * n + i] = v; }
};

RC_HD bool finite(double x) { return __builtin_fabs(x) <= 1.7976931348623157e308; }   // false for a NaN
RC_HD double quiet_nan() { return __builtin_nan(""); }

#if defined(__HIP_DEVICE_COMPILE__)
RC_HD double ieee_sqrt(double x) { return __dsqrt_rn(x); }
RC_HD double ieee_div(double a, double b) { return __ddiv_rn(a, b); }
#else
RC_HD double ieee_sqrt(double x) { return __builtin_sqrt(x); }
RC_HD double ieee_div(double a, double b) { return a / b; }
#endif

template <int NDIM>
RC_HD double dot(const double (&a)[NDIM], const double (&b)[NDIM]) {
    RCLB_NO_CONTRACT
    double acc = 0.0;
RCLB_UNROLL
    for (int i = 0; i < NDIM; ++i) {
        const double prod = a[i] * b[i];
        acc = acc + prod;
    }
    return acc;
}

template <int NDIM>
RC_HD double absmax(const double (&g)[NDIM]) {
    double acc = 0.0;
RCLB_UNROLL
    for (int i = 0; i < NDIM; ++i) {
        const double v = __builtin_fabs(g[i]);
        acc = v > acc ? v : acc;
    }
    return acc;
}

// min(1, 1 / ||g||_2)
template <int NDIM>
RC_HD double first_step(const double (&g)[NDIM]) {
    const double r = ieee_div(1.0, ieee_sqrt(dot<NDIM>(g, g)));
    return r < 1.0 ? r : 1.0;
}

// (ft, gt) of one row from the rows the gradient entries write: a[0 .. NDIM], b[0 .. NDIM] (kind 2 only), both with stride 1
template <int NDIM>
RC_HD void objective(int kind, double lam, const double* a, const double* b, double& ft, double (&gt)[NDIM]) {
    RCLB_NO_CONTRACT
    if (kind == kRaw) {
        ft = a[0];
RCLB_UNROLL
        for (int i = 0; i < NDIM; ++i) gt[i] = a[1 + i];
    } else if (kind == kOneMinus) {
        ft = 1.0 - a[0];
RCLB_UNROLL
        for (int i = 0; i < NDIM; ++i) gt[i] = -a[1 + i];
    } else {
        const double fav = a[0], m2 = b[0];
        const double sq = fav * fav;
        double var = m2 - sq;
        const double lim = kVarFloor * m2;
        const bool floor = var <= lim;
        var = floor ? 0.0 : var;
        const double sd = ieee_sqrt(var);
        const double safe2 = 2.0 * (floor ? 1.0 : sd);
RCLB_UNROLL
        for (int i = 0; i < NDIM; ++i) {
            const double fg = fav * a[1 + i];
            const double grad_var = 2.0 * (b[1 + i] - fg);
            const double grad_std = floor ? 0.0 : ieee_div(grad_var, safe2);
            const double term = lam * grad_std;
            gt[i] = -a[1 + i] + term;
        }
        const double ls = lam * sd;
        ft = (1.0 - fav) + ls;
    }
}

// P(v): a NaN stays a NaN
RC_HD double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// lo == nullptr: the unbounded machine; otherwise the boxed one (lo and hi both given): x0 is projected, bad bounds end the row
template <class Row>
RC_HD void init_row_t(const Row& r, const Layout& L, const double* x0, const double* mask, const double* lo, const double* hi) {
    bool bad = false;
    for (int i = 0; i < L.n; ++i) {
        double v = x0[i];
        bad |= v != v;
        if (lo) {
            bad |= lo[i] != lo[i] || hi[i] != hi[i] || lo[i] > hi[i];
            v = clip(v, lo[i], hi[i]);
        }
        r.st(L.x() + i, v);
        r.st(L.g() + i, quiet_nan());
        r.st(L.d() + i, 0.0);
        r.st(L.mask() + i, mask ? mask[i] : 1.0);
    }
    for (int i = 0; i < L.n; ++i) r.trial_st(i, bad ? quiet_nan() : (lo ? clip(x0[i], lo[i], hi[i]) : x0[i]));
    for (int k = 0; k < L.m * L.n; ++k) {
        r.st(L.S() + k, 0.0);
        r.st(L.Y() + k, 0.0);
    }
    for (int k = 0; k < L.m; ++k) r.st(L.sy() + k, 0.0);
    r.st(L.f(), quiet_nan());
    r.st(L.t(), 0.0);
    r.st(L.gd(), 0.0);
    r.st(L.count(), 0.0);
    r.st(L.head(), 0.0);
    r.st(L.nback(), 0.0);
    r.st(L.iters(), 0.0);
    r.st(L.evals(), 0.0);
    r.st(L.fprev(), quiet_nan());
    r.st(L.status(), bad ? 5.0 : 0.0);
    r.st(L.first(), 1.0);
}

template <class Row>
RC_HD void init_row(const Row& r, const Layout& L, const double* x0, const double* mask) {
    init_row_t(r, L, x0, mask, nullptr, nullptr);
}

template <class Row>
RC_HD void init_row_box(const Row& r, const Layout& L, const double* x0, const double* mask, const double* lo, const double* hi) {
    init_row_t(r, L, x0, mask, lo, hi);
}

// x + t d into the trial row
template <int NDIM, class Row>
RC_HD void write_trial(const Row& r, const double (&x)[NDIM], double t, const double (&d)[NDIM]) {
    RCLB_NO_CONTRACT
RCLB_UNROLL
    for (int i = 0; i < NDIM; ++i) {
        const double step = t * d[i];
        r.trial_st(i, x[i] + step);
    }
}

// P(x + t d) into the trial row
template <int NDIM, class Row>
RC_HD void write_trial_box(const Row& r, const double (&x)[NDIM], double t, const double (&d)[NDIM], const double (&lo)[NDIM],
                           const double (&hi)[NDIM]) {
    RCLB_NO_CONTRACT
RCLB_UNROLL
    for (int i = 0; i < NDIM; ++i) {
        const double step = t * d[i];
        r.trial_st(i, clip(x[i] + step, lo[i], hi[i]));
    }
}

template <int NDIM, class Row>
RC_HD void finish_row(const Row& r, const Layout& L, int status) {
    r.st(L.status(), (double)status);
RCLB_UNROLL
    for (int i = 0; i < NDIM; ++i) r.trial_st(i, quiet_nan());
}

// d = -g, gd = g.d, t = first_step(g), no history, nback = 0, and the trial point
template <int NDIM, class Row>
RC_HD void steepest(const Row& r, const Layout& L, const double (&x)[NDIM], const double (&g)[NDIM]) {
    double d[NDIM];
RCLB_UNROLL
    for (int i = 0; i < NDIM; ++i) {
        d[i] = -g[i];
        r.st(L.d() + i, d[i]);
    }
    const double t = first_step<NDIM>(g);
    r.st(L.gd(), dot<NDIM>(g, d));
    r.st(L.t(), t);
    r.st(L.count(), 0.0);
    r.st(L.head(), 0.0);
    r.st(L.nback(), 0.0);
    write_trial<NDIM>(r, x, t, d);
}

// the active set of a new direction: a variable on a bound whose gradient points out of the box
template <int NDIM>
RC_HD void active_set(const double (&x)[NDIM], const double (&g)[NDIM], const double (&lo)[NDIM], const double (&hi)[NDIM],
                      bool (&act)[NDIM], double (&gr)[NDIM]) {
RCLB_UNROLL
    for (int i = 0; i < NDIM; ++i) {
        act[i] = (x[i] <= lo[i] && g[i] > 0.0) || (x[i] >= hi[i] && g[i] < 0.0);
        gr[i] = act[i] ? 0.0 : g[i];
    }
}

// boxed: d = -gr (g with the active entries 0), gd = g.d, t = first_step(gr), no history, nback = 0, and the projected trial point
template <int NDIM, class Row>
RC_HD void steepest_box(const Row& r, const Layout& L, const double (&x)[NDIM], const double (&g)[NDIM], const double (&lo)[NDIM],
                        const double (&hi)[NDIM]) {
    bool act[NDIM];
    double gr[NDIM], d[NDIM];
    active_set<NDIM>(x, g, lo, hi, act, gr);
RCLB_UNROLL
    for (int i = 0; i < NDIM; ++i) {
        d[i] = -gr[i];
        r.st(L.d() + i, d[i]);
    }
    const double t = first_step<NDIM>(gr);
    r.st(L.gd(), dot<NDIM>(g, d));
    r.st(L.t(), t);
    r.st(L.count(), 0.0);
    r.st(L.head(), 0.0);
    r.st(L.nback(), 0.0);
    write_trial_box<NDIM>(r, x, t, d, lo, hi);
}

// One call of `advance` for one row: (ft, gt) evaluated at the row's trial point, gt not yet masked.  Every trip count is a
// compile-time constant; the ring is read at the run-time slot through the accessor, never through a local array.  BOX: the boxed
// variant, blo / bhi the row's [NDIM] bounds (read into registers once the row is known to run); otherwise they are not touched.
template <int NDIM, bool BOX, class Row>
RC_HD void advance_row_t(const Row& r, const Layout& L, const Params& p, double ft, double (&gt)[NDIM], const double* blo,
                         const double* bhi) {
    RCLB_NO_CONTRACT
    if (r.ld(L.status()) != 0.0) return;                    // done: frozen, its trial row is NaN already
    const int m = L.m;
    [[maybe_unused]] double lo[NDIM], hi[NDIM];
    if constexpr (BOX) {
RCLB_UNROLL
        for (int i = 0; i < NDIM; ++i) {
            lo[i] = blo[i];
            hi[i] = bhi[i];
        }
    }
    bool gfinite = true;
RCLB_UNROLL
    for (int i = 0; i < NDIM; ++i) {
        gt[i] = gt[i] * r.ld(L.mask() + i);
        gfinite = gfinite && finite(gt[i]);
    }
    r.st(L.evals(), r.ld(L.evals()) + 1.0);
    double x[NDIM], g[NDIM];
    bool moved;
    const bool first = r.ld(L.first()) != 0.0;
    if (first) {
        r.st(L.first(), 0.0);
        if (!(finite(ft) && gfinite)) {
            finish_row<NDIM>(r, L, 5);
            return;
        }
        moved = true;
    } else {
        const double f = r.ld(L.f());
        if constexpr (BOX) {                                // the slope along the projected step, which must go downhill
            double s[NDIM], go[NDIM];
RCLB_UNROLL
            for (int i = 0; i < NDIM; ++i) {
                s[i] = r.trial_ld(i) - r.ld(L.x() + i);
                go[i] = r.ld(L.g() + i);
            }
            const double gs = dot<NDIM>(go, s);
            const double slope = p.c1 * gs;
            moved = finite(ft) && gs < 0.0 && ft <= f + slope;
        } else {
            const double t = r.ld(L.t());
            const double ct = p.c1 * t;
            const double slope = ct * r.ld(L.gd());
            moved = finite(ft) && ft <= f + slope;
        }
        if (moved) {                                        // accept: the pair (s, y)
            double s[NDIM], y[NDIM];
RCLB_UNROLL
            for (int i = 0; i < NDIM; ++i) {
                s[i] = r.trial_ld(i) - r.ld(L.x() + i);
                y[i] = gt[i] - r.ld(L.g() + i);
            }
            const double ss = dot<NDIM>(s, s), yy = dot<NDIM>(y, y), sy = dot<NDIM>(s, y);
            const double es = kPairEps * ieee_sqrt(ss);
            const double bound = es * ieee_sqrt(yy);
            if (sy > 0.0 && sy >= bound) {
                const int head = (int)r.ld(L.head()), count = (int)r.ld(L.count());
RCLB_UNROLL
                for (int i = 0; i < NDIM; ++i) {
                    r.st(L.S() + head * NDIM + i, s[i]);
                    r.st(L.Y() + head * NDIM + i, y[i]);
                }
                r.st(L.sy() + head, sy);
                r.st(L.head(), (double)(head + 1 == m ? 0 : head + 1));
                r.st(L.count(), (double)(count + 1 < m ? count + 1 : m));
            }
            r.st(L.fprev(), f);
            r.st(L.iters(), r.ld(L.iters()) + 1.0);
        }
    }
    if (!moved) {                                           // reject: halve, or drop the history once, then give up
        const double nback = r.ld(L.nback()) + 1.0;
        r.st(L.nback(), nback);
RCLB_UNROLL
        for (int i = 0; i < NDIM; ++i) x[i] = r.ld(L.x() + i);
        if (nback > (double)p.maxback) {
            if (r.ld(L.count()) == 0.0) {
                finish_row<NDIM>(r, L, 4);
                return;
            }
RCLB_UNROLL
            for (int i = 0; i < NDIM; ++i) g[i] = r.ld(L.g() + i);
            if constexpr (BOX)
                steepest_box<NDIM>(r, L, x, g, lo, hi);
            else
                steepest<NDIM>(r, L, x, g);
            return;
        }
        const double t = r.ld(L.t()) * 0.5;
        r.st(L.t(), t);
        double d[NDIM];
RCLB_UNROLL
        for (int i = 0; i < NDIM; ++i) d[i] = r.ld(L.d() + i);
        if constexpr (BOX)
            write_trial_box<NDIM>(r, x, t, d, lo, hi);
        else
            write_trial<NDIM>(r, x, t, d);
        return;
    }
    // the trial point becomes the iterate
RCLB_UNROLL
    for (int i = 0; i < NDIM; ++i) {
        x[i] = r.trial_ld(i);
        g[i] = gt[i];
        r.st(L.x() + i, x[i]);
        r.st(L.g() + i, g[i]);
    }
    r.st(L.f(), ft);
    if constexpr (BOX) {                                    // the projected gradient x - P(x - g)
        double pg[NDIM];
RCLB_UNROLL
        for (int i = 0; i < NDIM; ++i) pg[i] = x[i] - clip(x[i] - g[i], lo[i], hi[i]);
        if (absmax<NDIM>(pg) <= p.gtol) {
            finish_row<NDIM>(r, L, 1);
            return;
        }
    } else {
        if (absmax<NDIM>(g) <= p.gtol) {
            finish_row<NDIM>(r, L, 1);
            return;
        }
    }
    if (!first) {
        const double fprev = r.ld(L.fprev());
        double big = __builtin_fabs(fprev);
        const double af = __builtin_fabs(ft);
        big = af > big ? af : big;
        big = 1.0 > big ? 1.0 : big;
        const double tol = p.ftol * big;
        if (p.ftol > 0.0 && fprev - ft <= tol) {
            finish_row<NDIM>(r, L, 2);
            return;
        }
        if (r.ld(L.iters()) >= (double)p.maxiter) {
            finish_row<NDIM>(r, L, 3);
            return;
        }
    }
    const int count = (int)r.ld(L.count()), head = (int)r.ld(L.head());
    if (count > 0) {
        double q[NDIM], alpha[kMaxM];
        [[maybe_unused]] bool act[NDIM];
        if constexpr (BOX) {
            active_set<NDIM>(x, g, lo, hi, act, q);
        } else {
RCLB_UNROLL
            for (int i = 0; i < NDIM; ++i) q[i] = g[i];
        }
RCLB_UNROLL
        for (int j = 0; j < kMaxM; ++j) {                   // newest first
            alpha[j] = 0.0;
            if (j < count) {
                int slot = head - 1 - j;
                if (slot < 0) slot += m;
                double acc = 0.0;
RCLB_UNROLL
                for (int i = 0; i < NDIM; ++i) {
                    const double prod = r.ld(L.S() + slot * NDIM + i) * q[i];
                    acc = acc + prod;
                }
                const double a = ieee_div(1.0, r.ld(L.sy() + slot)) * acc;
                alpha[j] = a;
RCLB_UNROLL
                for (int i = 0; i < NDIM; ++i) {
                    const double prod = a * r.ld(L.Y() + slot * NDIM + i);
                    q[i] = q[i] - prod;
                }
            }
        }
        {
            const int newest = head - 1 < 0 ? head - 1 + m : head - 1;
            double yy = 0.0;
RCLB_UNROLL
            for (int i = 0; i < NDIM; ++i) {
                const double v = r.ld(L.Y() + newest * NDIM + i);
                const double prod = v * v;
                yy = yy + prod;
            }
            const double h0 = ieee_div(r.ld(L.sy() + newest), yy);
RCLB_UNROLL
            for (int i = 0; i < NDIM; ++i) q[i] = h0 * q[i];
        }
RCLB_UNROLL
        for (int jj = 0; jj < kMaxM; ++jj) {                // oldest first
            const int j = kMaxM - 1 - jj;
            if (j < count) {
                int slot = head - 1 - j;
                if (slot < 0) slot += m;
                double acc = 0.0;
RCLB_UNROLL
                for (int i = 0; i < NDIM; ++i) {
                    const double prod = r.ld(L.Y() + slot * NDIM + i) * q[i];
                    acc = acc + prod;
                }
                const double b = ieee_div(1.0, r.ld(L.sy() + slot)) * acc;
                const double w = alpha[j] - b;
RCLB_UNROLL
                for (int i = 0; i < NDIM; ++i) {
                    const double prod = w * r.ld(L.S() + slot * NDIM + i);
                    q[i] = q[i] + prod;
                }
            }
        }
        double d[NDIM];
RCLB_UNROLL
        for (int i = 0; i < NDIM; ++i) {
            d[i] = -q[i];
            if constexpr (BOX) d[i] = act[i] ? 0.0 : d[i];
        }
        const double gd = dot<NDIM>(g, d);
        if (!(gd >= 0.0)) {
RCLB_UNROLL
            for (int i = 0; i < NDIM; ++i) r.st(L.d() + i, d[i]);
            r.st(L.gd(), gd);
            r.st(L.t(), 1.0);
            r.st(L.nback(), 0.0);
            if constexpr (BOX)
                write_trial_box<NDIM>(r, x, 1.0, d, lo, hi);
            else
                write_trial<NDIM>(r, x, 1.0, d);
            return;
        }
    }
    // no pair stored, or not a descent direction: drop the history
    if constexpr (BOX)
        steepest_box<NDIM>(r, L, x, g, lo, hi);
    else
        steepest<NDIM>(r, L, x, g);
}

template <int NDIM, class Row>
RC_HD void advance_row(const Row& r, const Layout& L, const Params& p, double ft, double (&gt)[NDIM]) {
    advance_row_t<NDIM, false>(r, L, p, ft, gt, nullptr, nullptr);
}

template <int NDIM, class Row>
RC_HD void advance_row_box(const Row& r, const Layout& L, const Params& p, double ft, double (&gt)[NDIM], const double* lo,
                           const double* hi) {
    advance_row_t<NDIM, true>(r, L, p, ft, gt, lo, hi);
}

}  // namespace rclb
