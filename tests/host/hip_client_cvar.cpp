// CVaR of the fidelity and its gradient from a HIP host program - no Python, no torch: the three enqueue-only entries of the C ABI
// (include/robchar_hip.h) behind each other on the program's own stream, nothing synchronised until the copy back:
//   rc_mc_fidelity_philox_f64_async       the fidelities of all K counter-based draws of every controller
//   rc_tail_select_f64_async              list, weights and value at risk of the worst ceil(alpha K) of them
//   rc_mc_fidelity_grad_listed_f64_async  the weighted gradient sums over the listed draws: (CVaR, d CVaR / dx)
// tests/test_cabi_tail_select.py builds it; tests/test_gpu_tail_select.py runs it and compares with fidelity_cvar_philox.
//   argv: N in out C K seed sigma alpha      stdin: C*(N+1) controller values
//   stdout: per controller one line: CVaR, its N + 1 gradient entries, the value at risk
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "robchar_hip.h"

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
#define RCCHK(x) do { int r_ = (x); if (r_ != RC_OK) { fprintf(stderr, "%s: %d %s\n", #x, r_, rc_last_error()); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc != 9) return 2;
    const int N = atoi(argv[1]), in = atoi(argv[2]), out = atoi(argv[3]);
    const long long C = atoll(argv[4]), K = atoll(argv[5]);
    const unsigned long long seed = strtoull(argv[6], nullptr, 10);
    const double sigma = atof(argv[7]), alpha = atof(argv[8]);
    std::vector<double> ctrl((size_t)C * (N + 1));
    for (double& v : ctrl) if (scanf("%lf", &v) != 1) return 2;
    const long long m = rc_tail_select_len(K, alpha);
    if (m < 1) { fprintf(stderr, "rc_tail_select_len: %lld\n", m); return 1; }
    double *d_ctrl, *d_fid, *d_weight, *d_var, *d_sum;
    int* d_list;
    HIPCHK(hipMalloc(&d_ctrl, ctrl.size() * sizeof(double)));
    HIPCHK(hipMalloc(&d_fid, (size_t)C * K * sizeof(double)));
    HIPCHK(hipMalloc(&d_list, (size_t)C * m * sizeof(int)));
    HIPCHK(hipMalloc(&d_weight, (size_t)C * m * sizeof(double)));
    HIPCHK(hipMalloc(&d_var, (size_t)C * sizeof(double)));
    HIPCHK(hipMalloc(&d_sum, (size_t)C * (N + 2) * sizeof(double)));
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIPCHK(hipMemcpy(d_ctrl, ctrl.data(), ctrl.size() * sizeof(double), hipMemcpyHostToDevice));
    RCCHK(rc_mc_fidelity_philox_f64_async(0, st, RC_KERNEL_AUTO, N, in, out, nullptr, nullptr, d_ctrl, seed, 0ull, sigma, nullptr, C, K, d_fid));
    RCCHK(rc_tail_select_f64_async(0, st, d_fid, C, K, alpha, d_list, d_weight, d_var));
    RCCHK(rc_mc_fidelity_grad_listed_f64_async(0, st, N, in, out, nullptr, nullptr, d_ctrl, seed, 0ull, sigma, nullptr, 0, C, K, d_list,
                                               d_weight, m, nullptr, nullptr, d_sum));
    std::vector<double> sum((size_t)C * (N + 2)), var((size_t)C);
    HIPCHK(hipMemcpyAsync(sum.data(), d_sum, sum.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(var.data(), d_var, var.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (long long c = 0; c < C; ++c) {
        for (int j = 0; j < N + 2; ++j) printf("%.17g ", sum[(size_t)c * (N + 2) + j]);
        printf("%.17g\n", var[(size_t)c]);
    }
    return 0;
}
