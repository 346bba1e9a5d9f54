// Randomised quasi-Monte Carlo from a HIP host program - no Python, no torch: the Sobol entries of the C ABI (include/robchar_hip.h)
// on the program's own stream, nothing synchronised until the copy back:
//   rc_sobol_dirnum_u32              the unscrambled Joe-Kuo table of the 3 N dimensions (host only), copied R times
//   rc_draws_sobol_f64_async         the normals of all K = R P samples of every controller as the [C][K][N][3] draw tensor
//   rc_mc_fidelity_f64_async         the tensor kernel on it
//   rc_mc_fidelity_sobol_f64_async   the same fidelities with the points generated inside the kernel
// The replicates differ by a digital shift alone, shift[r][d] = 2654435761 (r D + d + 1) mod 2^32, shared by the controllers.
// tests/test_cabi_sobol.py builds it; tests/test_gpu_sobol.py runs it and compares with backend.mc_fidelity_sobol.
//   argv: N in out C R P skip sigma      stdin: C*(N+1) controller values
//   stdout: "identical 1" when the two routes agree bit for bit, then per controller one line: its R replicate means
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "robchar_hip.h"

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
#define RCCHK(x) do { int r_ = (x); if (r_ != RC_OK) { fprintf(stderr, "%s: %d %s\n", #x, r_, rc_last_error()); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc != 9) return 2;
    const int N = atoi(argv[1]), in = atoi(argv[2]), out = atoi(argv[3]), R = atoi(argv[5]);
    const long long C = atoll(argv[4]), P = atoll(argv[6]), skip = atoll(argv[7]), K = R * P;
    const double sigma = atof(argv[8]);
    const int D = 3 * N;
    std::vector<double> ctrl((size_t)C * (N + 1));
    for (double& v : ctrl) if (scanf("%lf", &v) != 1) return 2;
    std::vector<unsigned int> dirnum((size_t)R * D * 32), shift((size_t)R * D);
    RCCHK(rc_sobol_dirnum_u32(D, dirnum.data()));
    for (int r = 1; r < R; ++r) memcpy(&dirnum[(size_t)r * D * 32], dirnum.data(), (size_t)D * 32 * sizeof(unsigned int));
    for (size_t i = 0; i < shift.size(); ++i) shift[i] = 2654435761u * (unsigned int)(i + 1);
    double *d_ctrl, *d_draws, *d_two, *d_fused;
    unsigned int *d_dirnum, *d_shift;
    HIPCHK(hipMalloc(&d_ctrl, ctrl.size() * sizeof(double)));
    HIPCHK(hipMalloc(&d_dirnum, dirnum.size() * sizeof(unsigned int)));
    HIPCHK(hipMalloc(&d_shift, shift.size() * sizeof(unsigned int)));
    HIPCHK(hipMalloc(&d_draws, (size_t)C * K * D * sizeof(double)));
    HIPCHK(hipMalloc(&d_two, (size_t)C * K * sizeof(double)));
    HIPCHK(hipMalloc(&d_fused, (size_t)C * K * sizeof(double)));
    hipStream_t st;
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIPCHK(hipMemcpy(d_ctrl, ctrl.data(), ctrl.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_dirnum, dirnum.data(), dirnum.size() * sizeof(unsigned int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_shift, shift.data(), shift.size() * sizeof(unsigned int), hipMemcpyHostToDevice));
    RCCHK(rc_draws_sobol_f64_async(0, st, D, d_dirnum, d_shift, 0, R, P, skip, sigma, nullptr, C, K, d_draws, nullptr));
    RCCHK(rc_mc_fidelity_f64_async(0, st, RC_KERNEL_AUTO, N, in, out, nullptr, nullptr, 0, d_ctrl, d_draws, C, K, d_two));
    RCCHK(rc_mc_fidelity_sobol_f64_async(0, st, RC_KERNEL_AUTO, N, in, out, nullptr, nullptr, d_ctrl, d_dirnum, d_shift, 0, R, P, skip, sigma,
                                         nullptr, C, K, d_fused));
    std::vector<double> two((size_t)C * K), fused((size_t)C * K);
    HIPCHK(hipMemcpyAsync(two.data(), d_two, two.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(fused.data(), d_fused, fused.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    printf("identical %d\n", memcmp(two.data(), fused.data(), two.size() * sizeof(double)) == 0 ? 1 : 0);
    for (long long c = 0; c < C; ++c) {
        for (int r = 0; r < R; ++r) {
            double s = 0.0;
            for (long long k = 0; k < P; ++k) s += fused[(size_t)(c * K + r * P + k)];
            printf("%.17g%c", s / (double)P, r + 1 < R ? ' ' : '\n');
        }
    }
    return 0;
}
