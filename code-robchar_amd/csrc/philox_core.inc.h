// The counter-based Gaussian stream, per element: Philox4x32-10 keyed by `seed`, counter (e >> 1) -> two 53-bit uniforms ->
// Box-Muller pair, element parity picks cos / sin (philox_pair, philox_element), with the two constant tables its table-driven
// ln and sin/cos read.  Shared by the generator kernel (k_draws.inc.h), the fidelity kernel that generates its own draws
// (k_fidelity_philox.inc.h) and the noise-sensitivity kernel that does (k_fidelity_sens_philox.inc.h): every one of them
// produces the same bits for the same element.
//
// #included INSIDE the anonymous namespace of a translation unit (robchar_hip.hip, robchar_large.hip through
// k_fidelity_chain.inc.h, robchar_grad.hip), after tridiag_core.h; every unit gets its own copy of the tables.
#pragma once

// (cos, sin)(2 pi k / 64), k = 0..63: source of the per-wave LDS copy that sincos_table reads
__device__ const double g_sincos_table[128] = {RC_SINCOS_TABLE_VALUES};

// a ^ b ^ c in ONE instruction (v_bitop3_b32, truth table 0x96; gfx950): the compiler leaves the two xors of a Philox round
// as two v_xor_b32 (round 4: 167 -> 152 VALU instructions per Box-Muller pair)
__device__ __forceinline__ unsigned int xor3(unsigned int a, unsigned int b, unsigned int c) {
#if __has_builtin(__builtin_amdgcn_bitop3_b32)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}

__device__ __forceinline__ void philox4x32_10(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3,
                                              unsigned int k0, unsigned int k1, unsigned int (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned int n0 = xor3((unsigned int)(p1 >> 32), c1, k0);
        const unsigned int n1 = (unsigned int)p1;
        const unsigned int n2 = xor3((unsigned int)(p0 >> 32), c3, k1);
        const unsigned int n3 = (unsigned int)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// (ln c_k, 1 / c_k), c_k = 1/2 + (k + 1) / 256, k = 0..127: ln f = ln c_k + log1p((f - c_k) / c_k) for f in [1/2, 1)
#define RC_LN_TABLE_VALUES \
    -0.6853650401178903, 1.9844961240310077, -0.6776429940239801, 1.9692307692307693, \
    -0.6699801212784109, 1.9541984732824427, -0.6623755218931916, 1.9393939393939394, \
    -0.6548283162578087, 1.9248120300751879, -0.6473376445286511, 1.9104477611940298, \
    -0.639902666041133, 1.8962962962962964, -0.6325225587435105, 1.8823529411764706, \
    -0.6251965186514375, 1.8686131386861313, -0.6179237593223578, 1.855072463768116, \
    -0.6107035113488707, 1.841726618705036, -0.6035350218702582, 1.8285714285714285, \
    -0.5964175541013942, 1.8156028368794326, -0.5893503868783018, 1.8028169014084507, \
    -0.5823328142196552, 1.7902097902097902, -0.5753641449035618, 1.7777777777777777, \
    -0.5684437020589881, 1.7655172413793103, -0.561570822771226, 1.7534246575342465, \
    -0.5547448577008262, 1.7414965986394557, -0.5479651707154474, 1.7297297297297298, \
    -0.5412311385341033, 1.7181208053691275, -0.5345421503833068, 1.7066666666666668, \
    -0.5278976076646381, 1.695364238410596, -0.5212969236332861, 1.6842105263157894, \
    -0.514739523087127, 1.673202614379085, -0.5082248420659333, 1.6623376623376624, \
    -0.5017523275603158, 1.6516129032258065, -0.4953214372300254, 1.641025641025641, \
    -0.4889316391312544, 1.6305732484076434, -0.48258241145259567, 1.620253164556962, \
    -0.47627324225933093, 1.610062893081761, -0.4700036292457356, 1.6, \
    -0.4637730794950995, 1.5900621118012421, -0.4575811092471784, 1.5802469135802468, \
    -0.4514272436728001, 1.5705521472392638, -0.44531101665536404, 1.5609756097560976, \
    -0.4392319705789819, 1.5515151515151515, -0.43318965612301924, 1.5421686746987953, \
    -0.42718363206280735, 1.532934131736527, -0.42121346507630353, 1.5238095238095237, \
    -0.415278729556489, 1.514792899408284, -0.4093790074293007, 1.5058823529411764, \
    -0.40351388797690263, 1.4970760233918128, -0.39768296766610944, 1.4883720930232558, \
    -0.39188584998178355, 1.4797687861271676, -0.38612214526503347, 1.471264367816092, \
    -0.38039147055604844, 1.4628571428571429, -0.3746934494414107, 1.4545454545454546, \
    -0.36902771190573336, 1.4463276836158192, -0.3633938941874773, 1.4382022471910112, \
    -0.3577916386388075, 1.4301675977653632, -0.3522205935893521, 1.4222222222222223, \
    -0.3466804132137367, 1.4143646408839778, -0.34117075740276714, 1.4065934065934067, \
    -0.33569129163814154, 1.3989071038251366, -0.33024168687057687, 1.391304347826087, \
    -0.32482161940123766, 1.3837837837837839, -0.3194307707663612, 1.3763440860215055, \
    -0.31406882762497584, 1.3689839572192513, -0.3087354816496133, 1.3617021276595744, \
    -0.3034304294199201, 1.3544973544973544, -0.29815337231907635, 1.3473684210526315, \
    -0.2929040164329326, 1.3403141361256545, -0.2876820724517809, 1.3333333333333333, \
    -0.2824872555746769, 1.3264248704663213, -0.27731928541623435, 1.3195876288659794, \
    -0.27217788591581565, 1.3128205128205128, -0.26706278524904525, 1.3061224489795917, \
    -0.26197371574157396, 1.299492385786802, -0.2569104137850272, 1.292929292929293, \
    -0.2518726197550701, 1.2864321608040201, -0.24686007793152578, 1.28, \
    -0.24187253642048673, 1.2736318407960199, -0.2369097470783577, 1.2673267326732673, \
    -0.23197146543777514, 1.2610837438423645, -0.22705745063534608, 1.2549019607843137, \
    -0.2221674653411543, 1.248780487804878, -0.2173012756899814, 1.2427184466019416, \
    -0.2124586512141934, 1.2367149758454106, -0.2076393647782445, 1.2307692307692308, \
    -0.20284319251475147, 1.2248803827751196, -0.1980699137620938, 1.2190476190476192, \
    -0.19331931100349597, 1.2132701421800949, -0.18859116980755003, 1.2075471698113207, \
    -0.18388527877013736, 1.2018779342723005, -0.179201429457711, 1.1962616822429906, \
    -0.17453941635189968, 1.1906976744186046, -0.16989903679539747, 1.1851851851851851, \
    -0.16528009093910292, 1.1797235023041475, -0.16068238169047347, 1.1743119266055047, \
    -0.15610571466306167, 1.1689497716894977, -0.15154989812720093, 1.1636363636363636, \
    -0.14701474296180966, 1.158371040723982, -0.14250006260728304, 1.1531531531531531, \
    -0.13800567301944372, 1.147982062780269, -0.13353139262452263, 1.1428571428571428, \
    -0.12907704227514236, 1.1377777777777778, -0.1246424452072766, 1.1327433628318584, \
    -0.1202274269981598, 1.1277533039647578, -0.1158318155251217, 1.1228070175438596, \
    -0.11145544092532282, 1.1179039301310043, -0.1070981355563671, 1.1130434782608696, \
    -0.10275973395776894, 1.1082251082251082, -0.09844007281325252, 1.103448275862069, \
    -0.09413899091386191, 1.0987124463519313, -0.08985632912186105, 1.0940170940170941, \
    -0.08559193033540351, 1.0893617021276596, -0.0813456394539524, 1.0847457627118644, \
    -0.07711730334443129, 1.080168776371308, -0.07290677080808779, 1.0756302521008403, \
    -0.06871389254805181, 1.0711297071129706, -0.06453852113757118, 1.0666666666666667, \
    -0.06038051098890748, 1.062240663900415, -0.05623971832287608, 1.0578512396694215, \
    -0.05211600113901402, 1.0534979423868314, -0.048009219186360606, 1.0491803278688525, \
    -0.04391923393483549, 1.0448979591836736, -0.039845908547199674, 1.0406504065040652, \
    -0.03578910785158528, 1.0364372469635628, -0.0317486983145803, 1.032258064516129, \
    -0.027724548014854862, 1.0281124497991967, -0.023716526617316044, 1.024, \
    -0.01972450534777859, 1.0199203187250996, -0.015748356968139168, 1.0158730158730158, \
    -0.01178795575204224, 1.0118577075098814, -0.007843177461025893, 1.0078740157480315, \
    -0.003913899321136329, 1.003921568627451, 0.0, 1.0
__device__ const double g_ln_table[256] = {RC_LN_TABLE_VALUES};

// ln u for u in (0, 1]: u = 2^e f, f in [1/2, 1); ln f = ln c_k + log1p((f - c_k) / c_k) with the 128-entry (ln c, 1/c)
// table above (in LDS) and a degree-7 series on |r| <= 1/128.  A few ulp from libm.
__device__ __forceinline__ double ln_table(double u, const double* lntab) {
    const double f = __builtin_amdgcn_frexp_mant(u);
    const int ex = __builtin_amdgcn_frexp_exp(u);
    const int k = (int)((__double2hiint(f) >> 13) & 127);            // top 7 fraction bits
    const double ck = 0.5 + (double)(k + 1) * 0x1.0p-8;
    const double r = (f - ck) * lntab[2 * k + 1];                    // in [-1/128, 0)
    double p = fma(r, 1.0 / 7.0, -1.0 / 6.0);
    p = fma(r, p, 0.2);
    p = fma(r, p, -0.25);
    p = fma(r, p, 1.0 / 3.0);
    p = fma(r, p, -0.5);
    p = fma(r * r, p, r);                                            // log1p(r)
    return fma((double)ex, 6.93147180559945286227e-01, lntab[2 * k] + p);
}

// Everything behind the Philox call: the two 53-bit integers (a, b) of a counter -> amp = scale * radius and (cos, sin) of the
// Box-Muller pair.  Its own routine so that chosen bit patterns can be fed in (tests/host/hip_math_probe.cpp): no seed reaches
// a = 2^53 - 1 short of a 2^64 search.
// u1 lies in (0, 1]: a + 0.5 is a tie for a = 2^53 - 1 and rounds to 2^53, u1 == 1, and ln_table(1.0) is exactly +0.0 (f = 1/2,
// ex = 1: ln c_0 + log1p(r) rounds to -RN(ln 2)).  sqrt_rsqrt(0) is NaN (0 times the infinite seed; measured: both elements of
// the pair NaN), so the radicand carries a nudge IN the fma that forms it - the smallest denormal, 2^-1074.  -2 lnu is an exact
// product and >= 4.4e-16 for every other a (a = 2^53 - 2: u1 = 1 - 2^-52), so the sum rounds back to -2 lnu bit for bit: no
// element of any stream changes but that one pair, whose radius becomes 2.2e-162 (measured; v_rsq_f64 takes denormals) where
// the definition (oracle/philox_host.py) has 0.  The fma replaces the multiplication and 2^-1074 is the INLINE constant 1 of a
// 64-bit operand (v_fma_f64 v, v, -2.0, 1): no instruction and no register more (1e-300 cost two VGPRs for the literal).
__device__ __forceinline__ void box_muller_pair(unsigned long long a, unsigned long long b, double scale, const double* lntab,
                                                const double* sctab, double& amp, double& cs, double& sn) {
    const double u1 = ((double)a + 0.5) * 0x1.0p-53;               // (0, 1]
    const double u2 = ((double)b + 0.5) * 0x1.0p-53;
    const double lnu = ln_table(u1, lntab);
    double rad, rinv;
    rc::sqrt_rsqrt(fma(-2.0, lnu, 0x1.0p-1074), rad, rinv);
    rc::sincos_table(64.0 * u2, sctab, sn, cs);                    // 64 u2 <= 64: far inside sincos_table's domain
    amp = scale * rad;
}

// Box-Muller pair of counter `ctr`: elements 2 ctr = amp * cs and 2 ctr + 1 = amp * sn of stream `seed` (amp = scale * radius).
// Shared by philox_normal_kernel and by the fidelity kernel that generates its own draws (k_fidelity_philox.inc.h): the two
// produce the same bits.
__device__ __forceinline__ void philox_pair(unsigned long long seed, unsigned long long ctr, double scale, const double* lntab,
                                            const double* sctab, double& amp, double& cs, double& sn) {
    unsigned int w[4];
    philox4x32_10((unsigned int)ctr, (unsigned int)(ctr >> 32), 0u, 0u, (unsigned int)seed, (unsigned int)(seed >> 32), w);
    const unsigned long long a = (((unsigned long long)w[1] << 32) | w[0]) >> 11;
    const unsigned long long b = (((unsigned long long)w[3] << 32) | w[2]) >> 11;
    box_muller_pair(a, b, scale, lntab, sctab, amp, cs, sn);
}

// element `e` of the stream on its own (rare paths only: one Philox call per element)
__device__ __forceinline__ double philox_element(unsigned long long seed, unsigned long long e, double scale, const double* lntab,
                                                 const double* sctab) {
    double amp, cs, sn;
    philox_pair(seed, e >> 1, scale, lntab, sctab, amp, cs, sn);
    double v = (e & 1ull) ? amp * sn : amp * cs;
    asm volatile("" : "+v"(v));                    // rounded product, never contracted into its consumer (philox_lane_draws)
    return v;
}

// The per-wave LDS copies of the two tables (sctab[128], lntab[256], both 16-byte aligned): lane l copies entry l of the first and
// entries l, l + 64 of the second as double2.  The barrier costs nothing with one wave per workgroup.
__device__ __forceinline__ void philox_stage_tables(int lane, double* sctab, double* lntab) {
    reinterpret_cast<double2*>(sctab)[lane] = reinterpret_cast<const double2*>(g_sincos_table)[lane];
    reinterpret_cast<double2*>(lntab)[lane] = reinterpret_cast<const double2*>(g_ln_table)[lane];
    reinterpret_cast<double2*>(lntab)[lane + 64] = reinterpret_cast<const double2*>(g_ln_table)[lane + 64];
    __syncthreads();
}

// This lane's G consecutive elements of stream `seed` from element E on, into gl: what philox_normal_kernel would have stored
// there, bit for bit.  G / 2 + 1 Box-Muller pairs cover G elements from either parity of E (the pair grid straddles samples: one
// output of the first or of the last pair belongs to a neighbour).  Pair t = counter (E >> 1) + t holds the elements
// (2 t, 2 t + 1) after E when E is even and (2 t - 1, 2 t) when it is odd, so every gl[i] is a select between two VALUES of
// neighbouring pairs.  It is written that way, and not as v[i + odd] on an array of pair values, because a select between array
// elements becomes a load from a selected address: the array would go to scratch.
// The products amp * cs, amp * sn are rounded as philox_normal_kernel stores them and made opaque (__dmul_rn is a plain multiply
// to the optimiser): left to the compiler they would be contracted into the fma that forms the consumer's matrix entry - another
// rounding than the two-kernel route's, and the generated-draws kernels would no longer be bit-identical to it.
template <int G>
__device__ __forceinline__ void philox_lane_draws(unsigned long long seed, unsigned long long E, double scale, const double* lntab,
                                                  const double* sctab, double (&gl)[G]) {
    const unsigned long long c0 = E >> 1;
    const bool odd = (E & 1ull) != 0ull;
    double sn_prev = 0.0;
#pragma unroll
    for (int t = 0; t < G / 2 + 1; ++t) {
        double amp, cs, sn;
        philox_pair(seed, c0 + (unsigned long long)t, scale, lntab, sctab, amp, cs, sn);
        double a = amp * cs, b = amp * sn;
        asm volatile("" : "+v"(a), "+v"(b));
        if (2 * t < G) gl[2 * t] = odd ? b : a;
        if (t >= 1 && 2 * t - 1 < G) gl[2 * t - 1] = odd ? a : sn_prev;
        sn_prev = b;
    }
}
