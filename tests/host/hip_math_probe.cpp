// The hand-written fp64 primitives under every kernel, one at a time, on inputs chosen by the caller - no Python, no torch,
// nothing from the library: tridiag_core.h and philox_core.inc.h are compiled straight from csrc/.
//   hipcc -O1 --offload-arch=gfx950 -I code-robchar_amd/csrc   (tests/test_gpu_math.py): the device's primitives, hardware seeds;
//   g++ -O2 -ffp-contract=off -I code-robchar_amd/csrc         (tests/test_math_checks.py): the RC_HD primitives' host build
//                                                               (emulated +-5e-8 seeds), no GPU; ids 6 and 7 are refused.
//   argv: <input file> <output file>
//   input : records  { int64 id, int64 count, double param, payload }   payload = count doubles (ids 0..6) or count (a, b)
//           uint64 pairs (id 7); param = the draw scale of id 7, unused otherwise.  At most 20 000 inputs per record.
//   output: records  { int64 id, int64 count, int64 nd, int64 nh, count*nd doubles, count*nh doubles }: the first block is what
//           this build computes (device under hipcc, host under g++), the second - hipcc only, pure-IEEE primitives only
//           (sincos_table, sincos_reduced) - the host compilation of the same function in the same binary.
//   ids: 0 sincos_table(u) -> s, c      1 sincos_reduced(x) -> s, c     2 sqrt_rsqrt(x) -> root, inv    3 rcp_full(x)
//        4 seed_rsq(x)   5 seed_rcp(x)   6 ln_table(u)    7 box_muller_pair(a, b) -> amp, cs, sn, amp * cs, amp * sn
// One launch per record, tables in LDS filled as the product kernels fill them.  Every HIP call is checked; the first error ends
// the program with a non-zero status.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tridiag_core.h"

namespace {

constexpr long long kMaxCount = 20000;
constexpr int kIds = 8;
constexpr int kOutPerInput[kIds] = {2, 2, 2, 1, 1, 1, 1, 5};
constexpr bool kHostTwin[kIds] = {true, true, false, false, false, false, false, false};
const double kSinCosTable[128] = {RC_SINCOS_TABLE_VALUES};

// the RC_HD primitives as the host compiler builds them (ids 0..5)
void host_eval(int id, long long n, const double* x, double* o) {
    for (long long i = 0; i < n; ++i) {
        switch (id) {
        case 0: rc::sincos_table(x[i], kSinCosTable, o[2 * i], o[2 * i + 1]); break;
        case 1: rc::sincos_reduced(x[i], o[2 * i], o[2 * i + 1]); break;
        case 2: rc::sqrt_rsqrt(x[i], o[2 * i], o[2 * i + 1]); break;
        case 3: o[i] = rc::rcp_full(x[i]); break;
        case 4: o[i] = rc::seed_rsq(x[i]); break;
        default: o[i] = rc::seed_rcp(x[i]); break;
        }
    }
}

#if defined(__HIPCC__)
#include "philox_core.inc.h"

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__device__ __forceinline__ void fill_tables(double* sctab, double* lntab) {
    if (threadIdx.x < 64)
        reinterpret_cast<double2*>(sctab)[threadIdx.x] = reinterpret_cast<const double2*>(g_sincos_table)[threadIdx.x];
    if (threadIdx.x < 128)
        reinterpret_cast<double2*>(lntab)[threadIdx.x] = reinterpret_cast<const double2*>(g_ln_table)[threadIdx.x];
    __syncthreads();
}

// in: n doubles (ids 0..6) or 2 n uint64 (id 7); out: n * kOutPerInput[ID] doubles
template <int ID>
__global__ __launch_bounds__(256) void probe_kernel(const void* in, double* out, int n, double param) {
    __shared__ __attribute__((aligned(16))) double sctab[128];
    __shared__ __attribute__((aligned(16))) double lntab[256];
    fill_tables(sctab, lntab);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = ID == 7 ? 0.0 : static_cast<const double*>(in)[i];
    if (ID == 0) rc::sincos_table(x, sctab, out[2 * i], out[2 * i + 1]);
    if (ID == 1) rc::sincos_reduced(x, out[2 * i], out[2 * i + 1]);
    if (ID == 2) rc::sqrt_rsqrt(x, out[2 * i], out[2 * i + 1]);
    if (ID == 3) out[i] = rc::rcp_full(x);
    if (ID == 4) out[i] = rc::seed_rsq(x);
    if (ID == 5) out[i] = rc::seed_rcp(x);
    if (ID == 6) out[i] = ln_table(x, lntab);
    if (ID == 7) {
        const unsigned long long* ab = static_cast<const unsigned long long*>(in);
        double amp, cs, sn;
        box_muller_pair(ab[2 * i], ab[2 * i + 1], param, lntab, sctab, amp, cs, sn);
        out[5 * i] = amp;
        out[5 * i + 1] = cs;
        out[5 * i + 2] = sn;
        out[5 * i + 3] = amp * cs;                 // the two elements, as the generator kernel forms them
        out[5 * i + 4] = amp * sn;
    }
}

template <int ID>
int launch_one(const void* in, double* out, int n, double param) {
    hipLaunchKernelGGL(probe_kernel<ID>, dim3((n + 255) / 256), dim3(256), 0, 0, in, out, n, param);
    HIPCHK(hipGetLastError());
    return 0;
}

int device_eval(int id, long long n, const void* payload, size_t payload_bytes, double param, double* o) {
    void* d_in = nullptr;
    double* d_out = nullptr;
    const size_t out_bytes = (size_t)n * kOutPerInput[id] * sizeof(double);
    HIPCHK(hipMalloc(&d_in, payload_bytes));
    HIPCHK(hipMalloc(&d_out, out_bytes));
    HIPCHK(hipMemcpy(d_in, payload, payload_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(d_out, 0xff, out_bytes));                      // NaN wherever a kernel writes nothing
    int rc = 1;
    switch (id) {
    case 0: rc = launch_one<0>(d_in, d_out, (int)n, param); break;
    case 1: rc = launch_one<1>(d_in, d_out, (int)n, param); break;
    case 2: rc = launch_one<2>(d_in, d_out, (int)n, param); break;
    case 3: rc = launch_one<3>(d_in, d_out, (int)n, param); break;
    case 4: rc = launch_one<4>(d_in, d_out, (int)n, param); break;
    case 5: rc = launch_one<5>(d_in, d_out, (int)n, param); break;
    case 6: rc = launch_one<6>(d_in, d_out, (int)n, param); break;
    case 7: rc = launch_one<7>(d_in, d_out, (int)n, param); break;
    }
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(o, d_out, out_bytes, hipMemcpyDeviceToHost));
    HIPCHK(hipFree(d_in));
    HIPCHK(hipFree(d_out));
    return 0;
}
#endif

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
bool write_exact(FILE* f, const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <input> <output>\n", argv[0]);
        return 2;
    }
    FILE* fin = fopen(argv[1], "rb");
    FILE* fout = fopen(argv[2], "wb");
    if (!fin || !fout) {
        fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
        return 2;
    }
    for (;;) {
        long long head[2];
        double param;
        const size_t got = fread(head, 1, sizeof(head), fin);
        if (got == 0) break;                                         // end of the records
        if (got != sizeof(head) || !read_exact(fin, &param, sizeof(param))) {
            fprintf(stderr, "truncated record header\n");
            return 2;
        }
        const long long id = head[0], n = head[1];
        if (id < 0 || id >= kIds || n < 1 || n > kMaxCount) {
            fprintf(stderr, "bad record: id %lld count %lld\n", id, n);
            return 2;
        }
        const size_t payload_bytes = (size_t)n * (id == 7 ? 16 : 8);
        std::vector<unsigned char> payload(payload_bytes);
        if (!read_exact(fin, payload.data(), payload_bytes)) {
            fprintf(stderr, "truncated payload of record id %lld\n", id);
            return 2;
        }
        const int nd = kOutPerInput[id];
        std::vector<double> first((size_t)n * nd), second;
#if defined(__HIPCC__)
        if (device_eval((int)id, n, payload.data(), payload_bytes, param, first.data())) return 1;
        if (kHostTwin[id]) {
            second.resize((size_t)n * nd);
            host_eval((int)id, n, reinterpret_cast<const double*>(payload.data()), second.data());
        }
#else
        if (id > 5) {
            fprintf(stderr, "id %lld is a device-only primitive\n", id);
            return 3;
        }
        (void)kHostTwin;
        host_eval((int)id, n, reinterpret_cast<const double*>(payload.data()), first.data());
#endif
        const long long ohead[4] = {id, n, nd, second.empty() ? 0 : nd};
        if (!write_exact(fout, ohead, sizeof(ohead)) || !write_exact(fout, first.data(), first.size() * sizeof(double)) ||
            !write_exact(fout, second.data(), second.size() * sizeof(double))) {
            fprintf(stderr, "short write\n");
            return 2;
        }
    }
    fclose(fin);
    if (fclose(fout) != 0) return 2;
    return 0;
}
