// s2m_device.hpp — the device helpers of the registration path that more than one of its kernel headers uses: address-space
// casts, the grid's cell arithmetic, the host libm's sinf / cosf / atanf / hypotf restated, the DPP wave reductions, the
// transform of a pose.  Included by s2m_prep.hpp (map index and scan ordering), s2m_kernels.hpp /
// s2m_register.hpp (the LM loop), s2m_sc.hip (ScanContext) and s2m_abi_debug.hip (the kernels that pin the restated libm);
// a helper that one of them alone uses lives with it.  Compiled with -ffp-contract=off (see s2m_kernels.hpp).
//
// Reference citations are file:line into jimmyshe/liorf (src/mapOptmization.cpp unless named).
#pragma once
#include <float.h>
#include <math.h>
#include <string.h>
#include "s2m_types.h"

#if defined(__HIPCC__)
#define S2M_HD __host__ __device__
#else
#define S2M_HD
#endif

namespace s2m {

// ------------------------------------------------------------------------------------------
// small device helpers
// ------------------------------------------------------------------------------------------
// Pointers fetched from the DevCtx block in memory are generic to the compiler, and generic
// (flat_*) loads return out of order, forcing vmcnt(0)+lgkmcnt(0) at every use. G() states
// that they point to global memory so that global_load/global_store with counted waits are used.
template <typename T> using gptr = __attribute__((address_space(1))) T*;
template <typename T> __device__ __forceinline__ gptr<T> G(T* p) { return (gptr<T>)p; }
typedef float v4f __attribute__((ext_vector_type(4)));
// The DevCtx block of a scan is written by tiny kernels between the loops and only read by the registration kernels: seen
// through the constant address space its fields - the buffer pointers above all - come by scalar loads into scalar
// registers (a generic pointer makes every one of them a vector load into a pair of vector registers, because some store
// of the kernel might alias it: sixteen registers per lane, and spills in the 128-register builds).
typedef const __attribute__((address_space(4))) DevCtx* CtxP;
__device__ __forceinline__ CtxP ctx_const(const DevCtx* p) { return (CtxP)p; }
__device__ __forceinline__ GridDesc grid_of(CtxP cp)
{
    GridDesc g;
    g.ox = cp->g.ox; g.oy = cp->g.oy; g.oz = cp->g.oz; g.inv_e = cp->g.inv_e; g.e = cp->g.e;
    g.nx = cp->g.nx; g.ny = cp->g.ny; g.nz = cp->g.nz; g.ncells = cp->g.ncells;
    return g;
}
__device__ __forceinline__ uint32_t f2ord(float f)
{
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int cell_coord(float v, float o, float inv_e, int n)
{
    float f = floorf((v - o) * inv_e);
    f = fminf(fmaxf(f, 0.0f), (float)(n - 1));      // NaN -> 0, +-inf -> edge cells
    return (int)f;
}

// ------------------------------------------------------------------------------------------
// sinf / cosf as glibc >= 2.28 computes them (sysdeps/ieee754/flt-32/s_sinf.c, s_cosf.c, s_sincosf.h;
// S. Nagy's implementation [ext]): the reference builds its transform with std::sin/std::cos of floats
// (pcl::getTransformation, :348-351, and the LM trig, :1170-1175), i.e. with the host's libm, and glibc's
// sinf is not correctly rounded - near 0.3 rad it is one ulp off the correctly rounded value for 3 % of
// the arguments.  One ulp in the transform is enough to flip a marginal correspondence, so the launches
// that rebuild the transform on the device use the same arithmetic: argument reduction by a scaled
// float-to-int conversion, degree-7 / degree-8 polynomials in fp64, one rounding to fp32 at the end.
// Checked against glibc 2.35's sinf/cosf on 2e7 random arguments in [-4, 4]: no mismatch, with or without
// FMA contraction of the polynomial; tests/test_parity_gpu.py::test_device_trig_is_the_hosts compares the
// device results with the test host's libm.  |x| >= 120 does not occur for a pose angle and takes the fp64
// library function.
// ------------------------------------------------------------------------------------------
// The reduction constants and the polynomial coefficients (glibc's __sincosf_table[2]: the second set has c0..c4 negated) are
// literals: instruction immediates on the device, where a table indexed at run time sits in memory and costs every caller a
// dependent load or two in the middle of the polynomial.
constexpr double kSincosfHpiInv = 0x1.45F306DC9C883p+23, kSincosfHpi = 0x1.921FB54442D18p0;
S2M_HD inline double sincosf_sign(int n) { return ((n ^ (n >> 1)) & 1) ? -1.0 : 1.0; }   // {1, -1, -1, 1}[n & 3]
S2M_HD inline uint32_t abstop12(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    return (u >> 20) & 0x7ffu;
}
// neg: the second coefficient set
S2M_HD inline float sinf_poly(double x, double x2, bool neg, int n)
{
    if ((n & 1) == 0) {
        const double ps1 = -0x1.555545995a603p-3, ps2 = 0x1.1107605230bc4p-7, ps3 = -0x1.994eb3774cf24p-13;
        const double x3 = x * x2, s1 = ps2 + x2 * ps3, x7 = x3 * x2, s = x + x3 * ps1;
        return (float)(s + x7 * s1);
    }
    const double pc0 = neg ? -0x1p0 : 0x1p0, pc1 = neg ? 0x1.ffffffd0c621cp-2 : -0x1.ffffffd0c621cp-2;
    const double pc2 = neg ? -0x1.55553e1068f19p-5 : 0x1.55553e1068f19p-5, pc3 = neg ? 0x1.6c087e89a359dp-10 : -0x1.6c087e89a359dp-10;
    const double pc4 = neg ? -0x1.99343027bf8c3p-16 : 0x1.99343027bf8c3p-16;
    const double x4 = x2 * x2, c2 = pc3 + x2 * pc4, c1 = pc0 + x2 * pc1, x6 = x4 * x2, c = c1 + x4 * pc2;
    return (float)(c + x6 * c2);
}
// which = 0: sinf(y), 1: cosf(y)
S2M_HD inline float glibc_sincosf(float y, int which)
{
    double x = (double)y;
    if (abstop12(y) < abstop12(0x1.921FB6p-1f)) {                      // |y| < pi/4
        if (abstop12(y) < abstop12(0x1p-12f)) return which ? 1.0f : y;
        return sinf_poly(x, x * x, false, which);
    }
    if (abstop12(y) < abstop12(120.0f)) {
        const double r = x * kSincosfHpiInv;                            // reduce_fast: quadrant in bits 24..31
        const int n = ((int32_t)r + 0x800000) >> 24;
        x = x - (double)n * kSincosfHpi;
        const double sgn = sincosf_sign(n);
        return sinf_poly(x * sgn, x * x, (n & 2) != 0, n ^ which);
    }
    return which ? (float)cos(x) : (float)sin(x);
}

// Both at once for the launches that rebuild the transform: one argument reduction, and the two polynomials (independent
// chains) side by side; glibc's sinf and cosf share the reduction and differ only in which polynomial they return.
S2M_HD inline void glibc_sincosf_both(float y, float& sn, float& cs)
{
    double x = (double)y;
    int n = 0;
    int tbl = 0;
    if (abstop12(y) < abstop12(0x1.921FB6p-1f)) {                      // |y| < pi/4
        if (abstop12(y) < abstop12(0x1p-12f)) { sn = y; cs = 1.0f; return; }
    } else if (abstop12(y) < abstop12(120.0f)) {
        const double r = x * kSincosfHpiInv;
        n = ((int32_t)r + 0x800000) >> 24;
        x = x - (double)n * kSincosfHpi;
        x = x * sincosf_sign(n);
        tbl = (n & 2) ? 1 : 0;
    } else { sn = (float)sin(x); cs = (float)cos(x); return; }
    const double x2 = x * x;
    const float a = sinf_poly(x, x2, tbl != 0, 0), b = sinf_poly(x, x2, tbl != 0, 1);
    sn = (n & 1) ? b : a;
    cs = (n & 1) ? a : b;
}

// atanf as glibc computes it (sysdeps/ieee754/flt-32/s_atanf.c: the fdlibm algorithm in fp32 [ext]; no FMA
// variant exists for it): SCManager's xy2theta (include/Scancontext.cpp:23-36) calls atan on a float, i.e. the
// host's atanf, and a sector index is the ceiling of the angle - one ulp decides on which side of a sector
// boundary a point falls.  Checked against glibc 2.35's atanf on 2e7 random arguments: no mismatch; the
// GPU tests compare whole descriptors with the oracle, which calls the host's libm.
S2M_HD inline float glibc_atanf(float x)
{
    const float atanhi[4] = { 4.6364760399e-01f, 7.8539812565e-01f, 9.8279368877e-01f, 1.5707962513e+00f };
    const float atanlo[4] = { 5.0121582440e-09f, 3.7748947079e-08f, 3.4473217170e-08f, 7.5497894159e-08f };
    const float aT[11] = { 3.3333334327e-01f, -2.0000000298e-01f, 1.4285714924e-01f, -1.1111110449e-01f, 9.0908870101e-02f, -7.6918758452e-02f,
                           6.6610731184e-02f, -5.8335702866e-02f, 4.9768779427e-02f, -3.6531571299e-02f, 1.6285819933e-02f };
    uint32_t u;
    memcpy(&u, &x, 4);
    const int32_t hx = (int32_t)u, ix = hx & 0x7fffffff;
    int id;
    if (ix >= 0x4c000000) {                              // |x| >= 2^25
        if (ix > 0x7f800000) return x + x;               // NaN
        return (hx > 0) ? atanhi[3] + atanlo[3] : -atanhi[3] - atanlo[3];
    }
    if (ix < 0x3ee00000) {                               // |x| < 0.4375
        if (ix < 0x31000000) return x;                   // |x| < 2^-29
        id = -1;
    } else {
        x = fabsf(x);
        if (ix < 0x3f980000) {                           // |x| < 1.1875
            if (ix < 0x3f300000) { id = 0; x = (2.0f * x - 1.0f) / (2.0f + x); }
            else                 { id = 1; x = (x - 1.0f) / (x + 1.0f); }
        } else {
            if (ix < 0x401c0000) { id = 2; x = (x - 1.5f) / (1.0f + 1.5f * x); }
            else                 { id = 3; x = -1.0f / x; }
        }
    }
    const float z = x * x, w = z * z;
    const float s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))));
    const float s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))));
    if (id < 0) return x - x * (s1 + s2);
    const float r = atanhi[id] - ((x * (s1 + s2) - atanlo[id]) - x);
    return (hx < 0) ? -r : r;
}

// hypotf as glibc computes it (sysdeps/ieee754/flt-32/e_hypotf.c [ext]: glibc >= 2.35 states it this way, older
// versions compute the same double expression): (float)sqrt((double)x * x + (double)y * y) with correctly rounded
// fp64 multiply, add and sqrt, and +inf for an infinite argument whatever the other one is.  cv::eigen's Jacobi
// rotations (eigen6_sym) call std::hypot on floats, i.e. the host's libm; the device library's hypotf scales by
// the larger exponent and works in fp32 (fma, then the fp32 square root), which is a different rounding: one ulp
// apart for about one argument pair in ten, and an ulp in a rotation moves the eigenvalues that the eig_thresh
// comparison reads.  The products are exact in fp64 (24-bit factors), so contraction could not change the sum;
// it stays unfused all the same.  tests/test_lm_close_gpu.py::test_device_hypot_is_the_hosts compares the device
// results with the test host's libm.
S2M_HD inline float glibc_hypotf(float x, float y)
{
    if (fabsf(x) == INFINITY || fabsf(y) == INFINITY) return INFINITY;
    const double dx = (double)x, dy = (double)y;
    const double xx = dx * dx, yy = dy * dy;
    return (float)sqrt(xx + yy);
}

// wave64 reductions / scan on the DPP cross-lane path (VALU rate, no LDS round trips):
// row_shr 1,2,4,8 inside the 16-lane rows, row_bcast:15 into rows 1 and 3, row_bcast:31 into
// rows 2 and 3; lane 63 then holds the result.  All 64 lanes must be active.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_i32(int old, int src)
{
    return __builtin_amdgcn_update_dpp(old, src, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f32(float old, float src)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_min_f32(float v)      // NaN-free inputs
{
    const float ID = INFINITY;
    v = fminf(v, dpp_f32<0x111, 0xf>(ID, v)); v = fminf(v, dpp_f32<0x112, 0xf>(ID, v));
    v = fminf(v, dpp_f32<0x114, 0xf>(ID, v)); v = fminf(v, dpp_f32<0x118, 0xf>(ID, v));
    v = fminf(v, dpp_f32<0x142, 0xa>(ID, v)); v = fminf(v, dpp_f32<0x143, 0xc>(ID, v));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_max_f32(float v)
{
    const float ID = -INFINITY;
    v = fmaxf(v, dpp_f32<0x111, 0xf>(ID, v)); v = fmaxf(v, dpp_f32<0x112, 0xf>(ID, v));
    v = fmaxf(v, dpp_f32<0x114, 0xf>(ID, v)); v = fmaxf(v, dpp_f32<0x118, 0xf>(ID, v));
    v = fmaxf(v, dpp_f32<0x142, 0xa>(ID, v)); v = fmaxf(v, dpp_f32<0x143, 0xc>(ID, v));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ int wave_max_i32(int v)
{
    constexpr int ID = (int)0x80000000;
    v = max(v, dpp_i32<0x111, 0xf>(ID, v)); v = max(v, dpp_i32<0x112, 0xf>(ID, v));
    v = max(v, dpp_i32<0x114, 0xf>(ID, v)); v = max(v, dpp_i32<0x118, 0xf>(ID, v));
    v = max(v, dpp_i32<0x142, 0xa>(ID, v)); v = max(v, dpp_i32<0x143, 0xc>(ID, v));
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t u)
{
    constexpr int ID = -1;                                   // 0xffffffff
    int v = (int)u;
    auto mn = [](int a, int b) { return (int)min((uint32_t)a, (uint32_t)b); };
    v = mn(v, dpp_i32<0x111, 0xf>(ID, v)); v = mn(v, dpp_i32<0x112, 0xf>(ID, v));
    v = mn(v, dpp_i32<0x114, 0xf>(ID, v)); v = mn(v, dpp_i32<0x118, 0xf>(ID, v));
    v = mn(v, dpp_i32<0x142, 0xa>(ID, v)); v = mn(v, dpp_i32<0x143, 0xc>(ID, v));
    return (uint32_t)__builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t u)
{
    int v = (int)u;
    v |= dpp_i32<0x111, 0xf>(0, v); v |= dpp_i32<0x112, 0xf>(0, v);
    v |= dpp_i32<0x114, 0xf>(0, v); v |= dpp_i32<0x118, 0xf>(0, v);
    v |= dpp_i32<0x142, 0xa>(0, v); v |= dpp_i32<0x143, 0xc>(0, v);
    return (uint32_t)__builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int wave_incl_scan_i32(int v)
{
    v += dpp_i32<0x111, 0xf>(0, v); v += dpp_i32<0x112, 0xf>(0, v);
    v += dpp_i32<0x114, 0xf>(0, v); v += dpp_i32<0x118, 0xf>(0, v);
    v += dpp_i32<0x142, 0xa>(0, v); v += dpp_i32<0x143, 0xc>(0, v);
    return v;
}

// transPointAssociateToMap (:1069-1072) and the LM trig (:1170-1175) from a pose: lanes 0..2 of the calling wave take one
// angle each (glibc's sinf / cosf arithmetic, see glibc_sincosf: what the host's libm would return); result in every lane.
__device__ __forceinline__ void build_transform(const float (&pose)[6], int lane, float (&T)[12], float (&sc6)[6])
{
    const float ang = (lane == 0) ? pose[2] : ((lane == 1) ? pose[1] : pose[0]);   // lane 0: yaw, 1: pitch, 2+: roll
    float snf, csf;
    glibc_sincosf_both(ang, snf, csf);
    const float B = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(snf), 0)), A = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(csf), 0));
    const float D = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(snf), 1)), C = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(csf), 1));
    const float F = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(snf), 2)), E = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(csf), 2));
    const float DE = D * E, DF = D * F;
    T[0] = A * C; T[1] = A * DF - B * E; T[2]  = B * F + A * DE; T[3]  = pose[3];
    T[4] = B * C; T[5] = A * E + B * DF; T[6]  = B * DE - A * F; T[7]  = pose[4];
    T[8] = -D;    T[9] = C * F;          T[10] = C * E;          T[11] = pose[5];
    sc6[0] = B; sc6[1] = A; sc6[2] = D; sc6[3] = C; sc6[4] = F; sc6[5] = E;
}

}  // namespace s2m
