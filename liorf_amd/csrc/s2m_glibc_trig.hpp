// s2m_glibc_trig.hpp — the host libm's sinf / cosf on the device, for the units that rebuild a transform the host also builds.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>

#define S2M_HD __host__ __device__

namespace s2m {
namespace {

// sinf / cosf as glibc >= 2.28 computes them: the arithmetic of s2m_device.hpp's glibc_sincosf_both, restated here because
// that header belongs to the registration path and its text is part of the stamp of the registration profiles (DESIGN.md
// section 14): the stages outside that path keep a copy of their own. Used by imageProjection's deskew (s2m_project.hip) and by the
// pose graph's correctPoses() (s2m_pose_graph.hip), which rebuilds the store's cached transforms as the host's libm would. tests/test_project_gpu.py compares every deskewed coordinate
// with a host build that calls libm: the ordinary cases stay below pi/4 (the polynomial alone), the *_large_rotations cases
// turn through several quadrants (the argument reduction). |angle| >= 120 rad, the fp64 library branch, is not exercised.
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
// sinf and cosf at once: one argument reduction, and the two polynomials (independent chains) side by side; glibc's sinf
// and cosf share the reduction and differ only in which polynomial they return.
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

}  // namespace
}  // namespace s2m
