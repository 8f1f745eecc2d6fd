// s2m_pose_graph.hip — kernels of the pose graph (saveKeyFramesAndFactor / correctPoses, reference
// src/mapOptmization.cpp:1386-1642), all fp64.  See s2m_pose_graph.hpp and DESIGN.md section 16.
#include "s2m_pose_graph.hpp"

#include <cmath>

#include "s2m_pose_readout.hpp"
#include "s2m_voxel.hpp"

namespace s2m {
namespace {

// ---- 3x3 / 6x6 helpers (row-major) -----------------------------------------------------------------------------
__device__ inline void m3_mul(const double* A, const double* B, double* C)       // C = A B
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
__device__ inline void m3_tmul(const double* A, const double* B, double* C)      // C = A^T B
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
__device__ inline void m3_tvec(const double* A, const double* v, double* o)      // o = A^T v
{
    for (int i = 0; i < 3; i++) o[i] = A[i] * v[0] + A[3 + i] * v[1] + A[6 + i] * v[2];
}
__device__ inline void m3_vec(const double* A, const double* v, double* o)
{
    for (int i = 0; i < 3; i++) o[i] = A[i * 3] * v[0] + A[i * 3 + 1] * v[1] + A[i * 3 + 2] * v[2];
}
__device__ inline void hat(const double* v, double* K)
{
    K[0] = 0; K[1] = -v[2]; K[2] = v[1]; K[3] = v[2]; K[4] = 0; K[5] = -v[0]; K[6] = -v[1]; K[7] = v[0]; K[8] = 0;
}
// I + a K + b K^2 with K = hat(v)
__device__ inline void rodrigues_form(const double* v, double a, double b, double* O)
{
    double K[9], K2[9];
    hat(v, K);
    m3_mul(K, K, K2);
    for (int i = 0; i < 9; i++) O[i] = a * K[i] + b * K2[i];
    O[0] += 1.0; O[4] += 1.0; O[8] += 1.0;
}
__device__ inline void so3_exp(const double* w, double* R)
{
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    if (th2 < 1e-20) { rodrigues_form(w, 1.0, 0.5, R); return; }
    const double th = sqrt(th2);
    rodrigues_form(w, sin(th) / th, (1.0 - cos(th)) / th2, R);
}
__device__ inline void so3_log(const double* R, double* phi)
{
    const double v[3] = { 0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1]) };
    const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    const double s = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (c < -0.99999) {                                  // near pi: the axis from the symmetric part, (1 - cos th) a_k a
        const double th = atan2(s, c);
        int k = 0;
        if (R[4] > R[0]) k = 1;
        if (R[8] > R[k * 4]) k = 2;
        double col[3] = { 0.5 * (R[k] + R[3 * k]), 0.5 * (R[3 + k] + R[3 * k + 1]), 0.5 * (R[6 + k] + R[3 * k + 2]) };
        col[k] -= c;
        const double nrm = sqrt(col[0] * col[0] + col[1] * col[1] + col[2] * col[2]);
        double sgn = (col[0] * v[0] + col[1] * v[1] + col[2] * v[2]) < 0.0 ? -1.0 : 1.0;
        for (int i = 0; i < 3; i++) phi[i] = th * sgn * col[i] / nrm;
        return;
    }
    const double f = s < 1e-10 ? 1.0 : atan2(s, c) / s;
    for (int i = 0; i < 3; i++) phi[i] = f * v[i];
}
__device__ inline void so3_jr_inv(const double* phi, double* J)
{
    const double th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
    if (th2 < 1e-10) { rodrigues_form(phi, 0.5, 1.0 / 12.0, J); return; }
    const double th = sqrt(th2);
    rodrigues_form(phi, 0.5, 1.0 / th2 - (1.0 + cos(th)) / (2.0 * th * sin(th)), J);
}
__device__ inline void so3_jr(const double* phi, double* J)
{
    const double th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
    if (th2 < 1e-10) { rodrigues_form(phi, -0.5, 1.0 / 6.0, J); return; }
    const double th = sqrt(th2);
    rodrigues_form(phi, -(1.0 - cos(th)) / th2, (th - sin(th)) / (th2 * th), J);
}

// [Log(R_E), t_E] of E = (Rr, tr)^-1 (R, t); Jinv = Jr^-1(phi), RE = R_E (the two diagonal blocks of D)
__device__ inline void local_of(const double* Rr, const double* tr, const double* R, const double* t, double* r, double* RE)
{
    m3_tmul(Rr, R, RE);
    const double d[3] = { t[0] - tr[0], t[1] - tr[1], t[2] - tr[2] };
    m3_tvec(Rr, d, r + 3);
    so3_log(RE, r);
}

__device__ inline void mat6_vec(const double* M, const double* v, double* o)
{
    for (int i = 0; i < 6; i++) {
        double a = 0.0;
        for (int j = 0; j < 6; j++) a += M[i * 6 + j] * v[j];
        o[i] = a;
    }
}
__device__ inline void mat6_tvec_add(const double* M, const double* v, double* o)  // o += M^T v
{
    for (int j = 0; j < 6; j++) {
        double a = 0.0;
        for (int i = 0; i < 6; i++) a += M[i * 6 + j] * v[i];
        o[j] += a;
    }
}

// One factor at the estimates X: raw residual r (rows), D blocks; writes the whitened (and robust-weighted) residual and
// Jacobian blocks, Dinv W^-1 when asked for, the error term and the weight.
__device__ void factor_eval(const PgFactor& f, const double* X, double* Ji, double* Jj, double* rw, double* Binv, double* err, double* wgt)
{
    double r[6] = { 0, 0, 0, 0, 0, 0 };
    double Di[36], Dj[36];
    for (int k = 0; k < 36; k++) Di[k] = Dj[k] = 0.0;
    double phi[3] = { 0, 0, 0 }, RE[9];
    const double* Xi = X + 12 * (size_t)f.i;
    if (f.type == kPgGps) {
        for (int a = 0; a < 3; a++) {
            r[a] = Xi[9 + a] - f.t[a];
            for (int b = 0; b < 3; b++) Di[a * 6 + 3 + b] = Xi[a * 3 + b];
        }
    } else {
        double D[36];
        for (int k = 0; k < 36; k++) D[k] = 0.0;
        double Rh[9], th[3];
        if (f.type == kPgPrior) {
            local_of(f.R, f.t, Xi, Xi + 9, r, RE);
        } else {
            const double* Xj = X + 12 * (size_t)f.j;
            m3_tmul(Xi, Xj, Rh);
            const double d[3] = { Xj[9] - Xi[9], Xj[10] - Xi[10], Xj[11] - Xi[11] };
            m3_tvec(Xi, d, th);
            local_of(f.R, f.t, Rh, th, r, RE);
        }
        phi[0] = r[0]; phi[1] = r[1]; phi[2] = r[2];
        double Jinv[9];
        so3_jr_inv(phi, Jinv);
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) { D[a * 6 + b] = Jinv[a * 3 + b]; D[(3 + a) * 6 + 3 + b] = RE[a * 3 + b]; }
        if (f.type == kPgPrior) {
            for (int k = 0; k < 36; k++) Di[k] = D[k];
        } else {
            for (int k = 0; k < 36; k++) Dj[k] = D[k];
            // Ji = -D Ad(h^-1), Ad(h^-1) = [[Rh^T, 0], [-Rh^T hat(th), Rh^T]]
            double Kh[9], RtK[9];
            hat(th, Kh);
            m3_tmul(Rh, Kh, RtK);
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) {
                    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
                    for (int c = 0; c < 3; c++) {
                        s0 += Jinv[a * 3 + c] * Rh[b * 3 + c];          // Jr^-1 Rh^T
                        s1 += RE[a * 3 + c] * RtK[c * 3 + b];           // RE Rh^T hat(th)
                        s2 += RE[a * 3 + c] * Rh[b * 3 + c];            // RE Rh^T
                    }
                    Di[a * 6 + b] = -s0;
                    Di[(3 + a) * 6 + b] = s1;
                    Di[(3 + a) * 6 + 3 + b] = -s2;
                }
        }
    }
    double e2 = 0.0;
    for (int a = 0; a < 6; a++) { r[a] = a < f.rows ? r[a] * f.sw[a] : 0.0; e2 += r[a] * r[a]; }
    double s = 1.0, w = 1.0;
    if (f.k > 0.0) {
        const double k2 = f.k * f.k;
        w = k2 / (k2 + e2);
        s = sqrt(w);
        *err = 0.5 * k2 * log1p(e2 / k2);
    } else {
        *err = 0.5 * e2;
    }
    *wgt = w;
    for (int a = 0; a < 6; a++) {
        const double m = a < f.rows ? f.sw[a] * s : 0.0;
        rw[a] = r[a] * s;
        for (int b = 0; b < 6; b++) {
            Ji[a * 6 + b] = Di[a * 6 + b] * m;
            if (Jj) Jj[a * 6 + b] = Dj[a * 6 + b] * m;
        }
    }
    if (Binv) {                                          // (W D)^-1 = blkdiag(Jr(phi), RE^T) W^-1; chain factors are never robust
        double Jr[9];
        so3_jr(phi, Jr);
        for (int k = 0; k < 36; k++) Binv[k] = 0.0;
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                Binv[a * 6 + b] = Jr[a * 3 + b] / f.sw[b];
                Binv[(3 + a) * 6 + 3 + b] = RE[b * 3 + a] / f.sw[3 + b];
            }
    }
}

// A kernel's gate (PgGate in the header), read before any other load: true = return at the head.
__device__ inline bool gated(PgGate g)
{
    return g.base && *reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(g.base) + blockIdx.y * g.stride);
}

__global__ void __launch_bounds__(kPgThreads) k_pg_linearize(PgDev d, const double* X, PgGate gate)
{
    if (gated(gate)) return;
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= d.n + d.n_extra) return;
    if (f < d.n) {
        const PgFactor fac = d.chain[f];
        double Ja[36], Jb[36];
        if (fac.type == kPgPrior) {                      // f == 0: B = the prior's block, no A
            factor_eval(fac, X, Ja, nullptr, d.rc + 6 * (size_t)f, d.Binv + 36 * (size_t)f, d.ferr + f, d.fw + f);
            for (int k = 0; k < 36; k++) d.Aof[36 * (size_t)f + k] = 0.0;
        } else {
            factor_eval(fac, X, Ja, Jb, d.rc + 6 * (size_t)f, d.Binv + 36 * (size_t)f, d.ferr + f, d.fw + f);
            for (int k = 0; k < 36; k++) d.Aof[36 * (size_t)f + k] = Ja[k];
        }
    } else {
        const int x = f - d.n;
        factor_eval(d.extra[x], X, d.Ji + 36 * (size_t)x, d.Jj + 36 * (size_t)x, d.rx + 6 * (size_t)x, nullptr, d.ferr + f, d.fw + f);
    }
}

// sum of the error terms and minimum of the weights, one workgroup, fixed order
__global__ void __launch_bounds__(kPgThreads) k_pg_err_reduce(PgDev d, PgGate gate)
{
    if (gated(gate)) return;
    __shared__ double se[kPgThreads], sw[kPgThreads];
    const int n = d.n + d.n_extra;
    double e = 0.0, w = 1.0;
    for (int k = threadIdx.x; k < n; k += kPgThreads) { e += d.ferr[k]; w = fmin(w, d.fw[k]); }
    se[threadIdx.x] = e; sw[threadIdx.x] = w;
    __syncthreads();
    for (int s = kPgThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { se[threadIdx.x] += se[threadIdx.x + s]; sw[threadIdx.x] = fmin(sw[threadIdx.x], sw[threadIdx.x + s]); }
        __syncthreads();
    }
    if (threadIdx.x == 0) { d.sc->err = se[0]; d.sc->wmin = sw[0]; }
}

// level-0 matrices of both scans: forward M_i = -Binv_i A_(i-1), C0 = Binv_i; transposed (e = n-1-i) M_e = -(A_i Binv_i)^T, C0 = Binv_i^T
__global__ void __launch_bounds__(kPgThreads) k_pg_scan_m0(PgDev d, PgGate gate)
{
    if (gated(gate)) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const double* B = d.Binv + 36 * (size_t)i;
    const double* A = d.Aof + 36 * (size_t)i;
    double* Mf = d.fwd.M[0] + 36 * (size_t)i;
    double* Cf = d.fwd.C0 + 36 * (size_t)i;
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++) {
            double s = 0.0;
            for (int c = 0; c < 6; c++) s += B[a * 6 + c] * A[c * 6 + b];
            Mf[a * 6 + b] = -s;
            Cf[a * 6 + b] = B[a * 6 + b];
        }
    const int e = d.n - 1 - i;
    double* Mb = d.bwd.M[0] + 36 * (size_t)e;
    double* Cb = d.bwd.C0 + 36 * (size_t)e;
    const double* An = d.Aof + 36 * (size_t)(i + 1);       // A_i: Jacobian of between(i, i+1) with respect to key i
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++) {
            double s = 0.0;
            if (i + 1 < d.n)
                for (int c = 0; c < 6; c++) s += An[b * 6 + c] * B[c * 6 + a];
            Mb[a * 6 + b] = -s;
            Cb[a * 6 + b] = B[b * 6 + a];
        }
}

// prefix products inside each group, one thread per (group, column); the group's product is the next level's matrix
__global__ void __launch_bounds__(kPgThreads) k_pg_scan_pre(const double* M, double* Pre, double* Mnext, int n, PgGate gate)
{
    if (gated(gate)) return;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int g = t / 6, col = t % 6;
    const int e0 = g * kPgGroup;
    if (e0 >= n) return;
    const int e1 = min(e0 + kPgGroup, n);
    double v[6] = { 0, 0, 0, 0, 0, 0 };
    v[col] = 1.0;
    for (int e = e0; e < e1; e++) {
        double o[6];
        mat6_vec(M + 36 * (size_t)e, v, o);
        for (int a = 0; a < 6; a++) { v[a] = o[a]; Pre[36 * (size_t)e + a * 6 + col] = o[a]; }
    }
    if (Mnext)
        for (int a = 0; a < 6; a++) Mnext[36 * (size_t)g + a * 6 + col] = v[a];
}

// ---- the linear solve: one family of kernels for one right-hand side (the optimise, s2m_pg_marginal) and for C of them in
// lockstep (PgCols in the header).  Column c = blockIdx.y: its vectors lie c * vec (u, loc) doubles behind column 0's, its
// kPgDotBlocks partials and its PgScalars c places on; Binv, M, Pre, C0, Ji, Jj are shared.  blockIdx.x and threadIdx.x
// have the same roles whatever the number of columns, so a column's sums run in one order.

// up-sweep, one thread per group: the group's recurrence from a zero input
__global__ void __launch_bounds__(64) k_pg_scan_up0(PgScan sc, size_t ls, const double* in, size_t vs, PgGate gate)
{
    if (gated(gate)) return;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = sc.n[0], e0 = g * kPgGroup;
    if (e0 >= n) return;
    const int e1 = min(e0 + kPgGroup, n);
    in += blockIdx.y * vs;
    double* loc0 = sc.loc[0] + blockIdx.y * ls;
    double v[6] = { 0, 0, 0, 0, 0, 0 };
    for (int e = e0; e < e1; e++) {
        const double* x = in + 6 * (size_t)(sc.rev ? n - 1 - e : e);
        const double xin[6] = { x[0], x[1], x[2], x[3], x[4], x[5] };
        double c[6], o[6];
        mat6_vec(sc.C0 + 36 * (size_t)e, xin, c);
        mat6_vec(sc.M[0] + 36 * (size_t)e, v, o);
        for (int a = 0; a < 6; a++) { v[a] = o[a] + c[a]; loc0[6 * (size_t)e + a] = v[a]; }
    }
}
__global__ void __launch_bounds__(64) k_pg_scan_up(PgScan sc, size_t ls, int lvl, PgGate gate)
{
    if (gated(gate)) return;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = sc.n[lvl], e0 = g * kPgGroup;
    if (e0 >= n) return;
    const int e1 = min(e0 + kPgGroup, n);
    const double* below = sc.loc[lvl - 1] + blockIdx.y * ls;
    double* here = sc.loc[lvl] + blockIdx.y * ls;
    double v[6] = { 0, 0, 0, 0, 0, 0 };
    for (int e = e0; e < e1; e++) {
        const int last = min(e * kPgGroup + kPgGroup, sc.n[lvl - 1]) - 1;
        const double* c = below + 6 * (size_t)last;
        double o[6];
        mat6_vec(sc.M[lvl] + 36 * (size_t)e, v, o);
        for (int a = 0; a < 6; a++) { v[a] = o[a] + c[a]; here[6 * (size_t)e + a] = v[a]; }
    }
}
// down-sweep, one thread per element: add the carry that enters the element's group
__global__ void __launch_bounds__(kPgThreads) k_pg_scan_down(PgScan sc, size_t ls, int lvl, double* out, size_t vs, PgGate gate)
{
    if (gated(gate)) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = sc.n[lvl];
    if (e >= n) return;
    const int g = e / kPgGroup;
    double* here = sc.loc[lvl] + blockIdx.y * ls;
    double v[6];
    for (int a = 0; a < 6; a++) v[a] = here[6 * (size_t)e + a];
    if (g > 0) {
        const double* xin = sc.loc[lvl + 1] + blockIdx.y * ls + 6 * (size_t)(g - 1);
        const double x6[6] = { xin[0], xin[1], xin[2], xin[3], xin[4], xin[5] };
        double o[6];
        mat6_vec(sc.Pre[lvl] + 36 * (size_t)e, x6, o);
        for (int a = 0; a < 6; a++) v[a] += o[a];
    }
    double* dst = lvl == 0 ? out + blockIdx.y * vs + 6 * (size_t)(sc.rev ? n - 1 - e : e) : here + 6 * (size_t)e;
    for (int a = 0; a < 6; a++) dst[a] = v[a];
}

// the extra factors: u_f = Ji x_i + Jj x_j; per key, in the order of its incidence list, g_k = sum J^T u
__global__ void __launch_bounds__(kPgThreads) k_pg_extra_u(PgDev d, PgCols s, const double* x, PgGate gate)
{
    if (gated(gate)) return;
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= d.n_extra) return;
    x += blockIdx.y * s.vec;
    double* u = d.u + blockIdx.y * s.u;
    const PgFactor& fac = d.extra[f];
    double xi[6], o[6], o2[6] = { 0, 0, 0, 0, 0, 0 };
    for (int a = 0; a < 6; a++) xi[a] = x[6 * (size_t)fac.i + a];
    mat6_vec(d.Ji + 36 * (size_t)f, xi, o);
    if (fac.type == kPgBetween) {
        for (int a = 0; a < 6; a++) xi[a] = x[6 * (size_t)fac.j + a];
        mat6_vec(d.Jj + 36 * (size_t)f, xi, o2);
    }
    for (int a = 0; a < 6; a++) u[6 * (size_t)f + a] = o[a] + o2[a];
}
__global__ void __launch_bounds__(kPgThreads) k_pg_extra_gather(PgDev d, PgCols s, PgGate gate)
{
    if (gated(gate)) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= d.n) return;
    const double* u = d.u + blockIdx.y * s.u;
    double* g = d.g + blockIdx.y * s.vec;
    double acc[6] = { 0, 0, 0, 0, 0, 0 };
    for (int q = d.inc_start[k]; q < d.inc_start[k + 1]; q++) {
        const PgIncidence in = d.inc[q];
        double uf[6];
        for (int a = 0; a < 6; a++) uf[a] = u[6 * (size_t)in.factor + a];
        mat6_tvec_add((in.side ? d.Jj : d.Ji) + 36 * (size_t)in.factor, uf, acc);
    }
    for (int a = 0; a < 6; a++) g[6 * (size_t)k + a] = acc[a];
}

// ---- CG vector steps: every sum in a fixed order (kPgDotBlocks x kPgThreads strided partials, then one thread).  The
// iteration's kernels return at their head once the column's sc->stop is set.
__device__ inline void block_partial(double a, double* partial)
{
    __shared__ double sm[kPgThreads];
    sm[threadIdx.x] = a;
    __syncthreads();
    for (int s = kPgThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sm[0];
}
__device__ inline double partial_sum(const double* partial)
{
    double s = 0.0;
    for (int k = 0; k < kPgDotBlocks; k++) s += partial[k];
    return s;
}

__global__ void __launch_bounds__(kPgThreads) k_pg_cg_init(PgDev d, PgCols s, PgGate gate)   // y = 0, r = p = b, partial of b.b
{
    if (gated(gate)) return;
    const size_t at = blockIdx.y * s.vec;
    const double* b = d.b + at;
    double *y = d.y + at, *r = d.r + at, *p = d.p + at;
    double a = 0.0;
    for (int k = blockIdx.x * kPgThreads + threadIdx.x; k < 6 * d.n; k += kPgDotBlocks * kPgThreads) {
        const double v = b[k];
        y[k] = 0.0; r[k] = v; p[k] = v;
        a += v * v;
    }
    block_partial(a, d.partial + blockIdx.y * kPgDotBlocks);
}
// (`close`: the launched optimise's head gate, shut behind the CG begin of a step that was opened; null otherwise)
__global__ void k_pg_cg_init2(PgDev d, double tol, int max_iters, PgGate gate, int32_t* close)
{
    if (gated(gate)) return;
    PgScalars* sc = d.sc + blockIdx.y;
    const double bb = partial_sum(d.partial + blockIdx.y * kPgDotBlocks);
    sc->rr = bb; sc->bb = bb; sc->tol2 = tol * tol;
    sc->iters = 0; sc->max_iters = max_iters;
    sc->stop = (bb == 0.0 || max_iters <= 0) ? 1 : 0;
    if (close) *close = 1;
}
__global__ void __launch_bounds__(kPgThreads) k_pg_cg_q(PgDev d, PgCols s, int have_t2)      // q = p + K^T K p, partial of p.q
{
    if (d.sc[blockIdx.y].stop) return;
    const size_t at = blockIdx.y * s.vec;
    const double *pv = d.p + at, *t2 = d.t2 + at;
    double* qv = d.q + at;
    double a = 0.0;
    for (int k = blockIdx.x * kPgThreads + threadIdx.x; k < 6 * d.n; k += kPgDotBlocks * kPgThreads) {
        const double p = pv[k], q = p + (have_t2 ? t2[k] : 0.0);
        qv[k] = q;
        a += p * q;
    }
    block_partial(a, d.partial + blockIdx.y * kPgDotBlocks);
}
__global__ void k_pg_cg_alpha(PgDev d)
{
    PgScalars* sc = d.sc + blockIdx.y;
    if (sc->stop) return;
    const double pq = partial_sum(d.partial + blockIdx.y * kPgDotBlocks);
    sc->pq = pq;
    sc->alpha = pq > 0.0 ? sc->rr / pq : 0.0;
}
__global__ void __launch_bounds__(kPgThreads) k_pg_cg_update(PgDev d, PgCols s)              // y += alpha p, r -= alpha q, partial of r.r
{
    if (d.sc[blockIdx.y].stop) return;
    const size_t at = blockIdx.y * s.vec;
    const double *pv = d.p + at, *qv = d.q + at;
    double *y = d.y + at, *rv = d.r + at;
    const double alpha = d.sc[blockIdx.y].alpha;
    double a = 0.0;
    for (int k = blockIdx.x * kPgThreads + threadIdx.x; k < 6 * d.n; k += kPgDotBlocks * kPgThreads) {
        y[k] += alpha * pv[k];
        const double r = rv[k] - alpha * qv[k];
        rv[k] = r;
        a += r * r;
    }
    block_partial(a, d.partial + blockIdx.y * kPgDotBlocks);
}
__global__ void k_pg_cg_beta(PgDev d)
{
    PgScalars* sc = d.sc + blockIdx.y;
    if (sc->stop) return;
    const double rr = partial_sum(d.partial + blockIdx.y * kPgDotBlocks);
    sc->beta = sc->rr > 0.0 ? rr / sc->rr : 0.0;
    sc->rr = rr;
    sc->iters += 1;
    if (!(rr > sc->tol2 * sc->bb) || sc->iters >= sc->max_iters || !(sc->pq > 0.0)) sc->stop = 1;
}
__global__ void __launch_bounds__(kPgThreads) k_pg_cg_p(PgDev d, PgCols s)
{
    if (d.sc[blockIdx.y].stop) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t at = blockIdx.y * s.vec;
    if (k < 6 * d.n) d.p[at + k] = d.r[at + k] + d.sc[blockIdx.y].beta * d.p[at + k];
}

__global__ void __launch_bounds__(kPgThreads) k_pg_unit(PgDev d, PgCols s, PgColAt at)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < 6 * d.n) d.g[blockIdx.y * s.vec + k] = k == at.v[blockIdx.y] ? 1.0 : 0.0;
}
// the wanted rows of every column's delta, so that one copy brings a pass's result to the host
__global__ void __launch_bounds__(64) k_pg_rows(PgDev d, PgCols s, PgColAt ka, PgColAt kb, double* rows)
{
    const int t = threadIdx.x;
    if (t >= 12) return;
    const int key = t < 6 ? ka.v[blockIdx.y] : kb.v[blockIdx.y];
    const bool in = key >= 0 && key < d.n;
    rows[12 * (size_t)blockIdx.y + t] = in ? d.delta[blockIdx.y * s.vec + 6 * (size_t)key + t % 6] : 0.0;
}

// ---- the step around the solve, on the graph's own vectors
__global__ void __launch_bounds__(kPgThreads) k_pg_rhs(PgDev d, int have_t2, PgGate gate)    // b = -(rc + t2)
{
    if (gated(gate)) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < 6 * d.n) d.b[k] = -(d.rc[k] + (have_t2 ? d.t2[k] : 0.0));
}
__global__ void __launch_bounds__(kPgThreads) k_pg_retract(PgDev d, PgGate gate)
{
    if (gated(gate)) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= d.n) return;
    const double* X = d.X + 12 * (size_t)i;
    const double* dl = d.delta + 6 * (size_t)i;
    const double w[3] = { dl[0], dl[1], dl[2] }, v[3] = { dl[3], dl[4], dl[5] };
    double E[9], Rn[9], Rv[3];
    so3_exp(w, E);
    m3_mul(X, E, Rn);
    m3_vec(X, v, Rv);
    double* O = d.Xtrial + 12 * (size_t)i;
    for (int k = 0; k < 9; k++) O[k] = Rn[k];
    for (int k = 0; k < 3; k++) O[9 + k] = X[9 + k] + Rv[k];
}
__global__ void __launch_bounds__(kPgThreads) k_pg_copy(const double* src, double* dst, int n, PgGate gate)
{
    if (gated(gate)) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) dst[k] = src[k];
}

// {x, y, z, roll, pitch, yaw} of Rot3::RzRyRx in float, and the store's position record
__global__ void __launch_bounds__(kPgThreads) k_pg_poses(const double* X, int first, int count, float* out, float4* pos)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    float* o = out + 6 * (size_t)k;
    pose_readout(X + 12 * (size_t)(first + k), o);
    if (pos) pos[k] = make_float4(o[0], o[1], o[2], 0.0f);
}

// correctPoses(), first half: per key the float pose vector of k_pg_poses and transCur = pcl::getTransformation of it (:317) in
// host_pose_to_transform's term order with the host libm's sinf / cosf (glibc_sincosf_both), 18 floats per key; *bad is set
// if an estimate is not finite.  Nothing of the store is touched yet.
__global__ void __launch_bounds__(kPgThreads) k_pg_store_stage(const double* X, int first, int count, float* stage, int32_t* bad)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    float o[6];
    pose_readout(X + 12 * (size_t)(first + k), o);
    bool ok = true;
    for (int a = 0; a < 6; a++) ok = ok && isfinite(o[a]);
    if (!ok) *bad = 1;
    float* q = stage + 18 * (size_t)k;
    for (int a = 0; a < 6; a++) q[a] = o[a];
    pose_transform(o, q + 6);
}
// second half: cloudKeyPoses3D and every key's cached transform from the staged values
__global__ void __launch_bounds__(kPgThreads) k_pg_store_write(const float* stage, int count, float4* pos, KfFrame* frames)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const float* q = stage + 18 * (size_t)k;
    pos[k] = make_float4(q[0], q[1], q[2], 0.0f);
    for (int a = 0; a < 12; a++) frames[k].T[a] = q[6 + a];
}

// ---- the launched optimise (s2m_pg_optimize_launch): the outer loop's decisions on the device.  PgRecord (in the header) holds
// the result and three gates, each "nonzero = return at the head": skip_head (rhs and CG begin of a step), skip_tail (the step,
// the trial point's linearisation and the close) and skip_keep (trial -> estimate).  The kernels of s2m_pg_optimize run between
// the four below with a record gate as their PgGate (the CG iterations stop by sc->stop as ever); no kernel waits for another.

// behind the linearisation at the launch-time estimates: the record of s2m_pg_optimize before its first step
__global__ void k_pg_open(PgDev d, PgRecord* rec, int max_iterations, double abs_tol, double rel_tol)
{
    const double err = d.sc->err;
    rec->iterations = 0; rec->inner_iterations = 0; rec->converged = 0;
    rec->max_iterations = max_iterations; rec->abs_tol = abs_tol; rec->rel_tol = rel_tol;
    rec->err = err; rec->error_before = err; rec->error_after = err; rec->wmin = d.sc->wmin;
    for (int k = 0; k < 12; k++) rec->A[k] = d.X[12 * (size_t)(d.n - 1) + k];
    rec->done = max_iterations <= 0 ? 1 : 0;
    rec->skip_head = rec->done; rec->skip_tail = 1; rec->skip_keep = 1;
}
// behind a chunk of CG iterations: the tail runs once the CG has stopped
__global__ void k_pg_gate(PgDev d, PgRecord* rec)
{
    rec->skip_tail = (rec->done || !d.sc->stop) ? 1 : 0;
    rec->skip_keep = 1;
}
// The close of a Gauss-Newton step, behind the trial point's linearisation: s2m_pg_optimize's comparisons in its order.
__global__ void k_pg_close(PgDev d, PgRecord* rec)
{
    if (rec->skip_tail) return;
    rec->inner_iterations += d.sc->iters;
    const double err_n = d.sc->err, err = rec->err;
    if (!(err_n < err)) { rec->converged = 1; rec->done = 1; return; }
    const double dec = err - err_n, old = err;
    rec->err = err_n;
    rec->iterations += 1;
    rec->error_after = err_n;
    rec->wmin = d.sc->wmin;
    rec->skip_keep = 0;
    for (int k = 0; k < 12; k++) rec->A[k] = d.Xtrial[12 * (size_t)(d.n - 1) + k];
    if (dec < rec->abs_tol || dec < rec->rel_tol * old) { rec->converged = 1; rec->done = 1; }
    else if (rec->iterations >= rec->max_iterations) rec->done = 1;
    else rec->skip_head = 0;
}
// a kept step: the trial point becomes the estimate
__global__ void __launch_bounds__(kPgThreads) k_pg_keep(PgDev d, const PgRecord* rec)
{
    if (rec->skip_keep) return;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < 12 * d.n) d.X[k] = d.Xtrial[k];
}

inline int blocks_for(int n) { return (n + kPgThreads - 1) / kPgThreads; }

// out = scan applied to in (both in key order), for every column (grid row = column); ls: c.loc_f or c.loc_b, the scan's
void scan_solve(hipStream_t s, const PgScan& sc, size_t ls, const double* in, double* out, const PgCols& c, PgGate gate)
{
    const unsigned C = (unsigned)c.cols;
    for (int l = 0; l < sc.levels; l++) {
        const int groups = (sc.n[l] + kPgGroup - 1) / kPgGroup;
        if (l == 0) k_pg_scan_up0<<<dim3((groups + 63) / 64, C), 64, 0, s>>>(sc, ls, in, c.vec, gate);
        else k_pg_scan_up<<<dim3((groups + 63) / 64, C), 64, 0, s>>>(sc, ls, l, gate);
    }
    for (int l = sc.levels - 2; l >= 1; l--) k_pg_scan_down<<<dim3(blocks_for(sc.n[l]), C), kPgThreads, 0, s>>>(sc, ls, l, out, c.vec, gate);
    k_pg_scan_down<<<dim3(blocks_for(sc.n[0]), C), kPgThreads, 0, s>>>(sc, ls, 0, out, c.vec, gate);
}

void scan_build(hipStream_t s, const PgScan& sc, PgGate gate)
{
    for (int l = 0; l < sc.levels; l++) {
        const int groups = (sc.n[l] + kPgGroup - 1) / kPgGroup;
        k_pg_scan_pre<<<blocks_for(groups * 6), kPgThreads, 0, s>>>(sc.M[l], sc.Pre[l], l + 1 < sc.levels ? sc.M[l + 1] : nullptr, sc.n[l], gate);
    }
}

// t2 = K^T u for the u already in d.u
void kt_apply(hipStream_t s, const PgDev& d, const PgCols& c, PgGate gate)
{
    k_pg_extra_gather<<<dim3(blocks_for(d.n), c.cols), kPgThreads, 0, s>>>(d, c, gate);
    scan_solve(s, d.bwd, c.loc_b, d.g, d.t2, c, gate);
}

bool cols_ok(const PgDev& d, const PgCols& c) { return d.n > 0 && c.cols >= 1 && c.cols <= kPgBlockCols; }

}  // namespace

hipError_t pg_linearize(hipStream_t s, const PgDev& d, const double* X, PgGate gate)
{
    if (d.n <= 0) return hipSuccess;
    k_pg_linearize<<<blocks_for(d.n + d.n_extra), kPgThreads, 0, s>>>(d, X, gate);
    k_pg_err_reduce<<<1, kPgThreads, 0, s>>>(d, gate);
    k_pg_scan_m0<<<blocks_for(d.n), kPgThreads, 0, s>>>(d, gate);
    scan_build(s, d.fwd, gate);
    scan_build(s, d.bwd, gate);
    return hipGetLastError();
}

hipError_t pg_rhs(hipStream_t s, const PgDev& d, PgGate gate)
{
    if (d.n_extra > 0) {
        k_pg_copy<<<blocks_for(6 * d.n_extra), kPgThreads, 0, s>>>(d.rx, d.u, 6 * d.n_extra, gate);
        kt_apply(s, d, kPgOne, gate);
    }
    k_pg_rhs<<<blocks_for(6 * d.n), kPgThreads, 0, s>>>(d, d.n_extra > 0, gate);
    return hipGetLastError();
}

hipError_t pg_step(hipStream_t s, const PgDev& d, PgGate gate)
{
    scan_solve(s, d.fwd, 0, d.y, d.delta, kPgOne, gate);
    k_pg_retract<<<blocks_for(d.n), kPgThreads, 0, s>>>(d, gate);
    return hipGetLastError();
}

hipError_t pg_retract(hipStream_t s, const PgDev& d)
{
    if (d.n <= 0) return hipErrorInvalidValue;
    k_pg_retract<<<blocks_for(d.n), kPgThreads, 0, s>>>(d, PgGate{});
    return hipGetLastError();
}

hipError_t pg_bwd_unit(hipStream_t s, const PgDev& d, const PgCols& c, const PgColAt& at)
{
    if (!cols_ok(d, c)) return hipErrorInvalidValue;
    k_pg_unit<<<dim3(blocks_for(6 * d.n), c.cols), kPgThreads, 0, s>>>(d, c, at);
    scan_solve(s, d.bwd, c.loc_b, d.g, d.b, c, PgGate{});
    return hipGetLastError();
}

hipError_t pg_cg_begin(hipStream_t s, const PgDev& d, const PgCols& c, double tol, int max_iters, PgGate gate, int32_t* close)
{
    if (!cols_ok(d, c)) return hipErrorInvalidValue;
    k_pg_cg_init<<<dim3(kPgDotBlocks, c.cols), kPgThreads, 0, s>>>(d, c, gate);
    k_pg_cg_init2<<<dim3(1, c.cols), 1, 0, s>>>(d, tol, max_iters, gate, close);
    return hipGetLastError();
}

hipError_t pg_cg_iterations(hipStream_t s, const PgDev& d, const PgCols& c, int count)
{
    if (!cols_ok(d, c)) return hipErrorInvalidValue;
    const unsigned C = (unsigned)c.cols;
    const PgGate stop{ &d.sc->stop, sizeof(PgScalars) };   // column c runs until its sc[c].stop
    for (int it = 0; it < count; it++) {
        if (d.n_extra > 0) {
            scan_solve(s, d.fwd, c.loc_f, d.p, d.t1, c, stop);
            k_pg_extra_u<<<dim3(blocks_for(d.n_extra), C), kPgThreads, 0, s>>>(d, c, d.t1, stop);
            kt_apply(s, d, c, stop);
        }
        k_pg_cg_q<<<dim3(kPgDotBlocks, C), kPgThreads, 0, s>>>(d, c, d.n_extra > 0);
        k_pg_cg_alpha<<<dim3(1, C), 1, 0, s>>>(d);
        k_pg_cg_update<<<dim3(kPgDotBlocks, C), kPgThreads, 0, s>>>(d, c);
        k_pg_cg_beta<<<dim3(1, C), 1, 0, s>>>(d);
        k_pg_cg_p<<<dim3(blocks_for(6 * d.n), C), kPgThreads, 0, s>>>(d, c);
    }
    return hipGetLastError();
}

hipError_t pg_fwd_y(hipStream_t s, const PgDev& d, const PgCols& c)
{
    if (!cols_ok(d, c)) return hipErrorInvalidValue;
    scan_solve(s, d.fwd, c.loc_f, d.y, d.delta, c, PgGate{});
    return hipGetLastError();
}

hipError_t pg_rows(hipStream_t s, const PgDev& d, const PgCols& c, const PgColAt& ka, const PgColAt& kb, double* rows)
{
    if (!cols_ok(d, c)) return hipErrorInvalidValue;
    k_pg_rows<<<dim3(1, c.cols), 64, 0, s>>>(d, c, ka, kb, rows);
    return hipGetLastError();
}

hipError_t pg_apply(hipStream_t s, const PgDev& d, const PgCols& c, int op)
{
    if (!cols_ok(d, c) || op < 0 || op > 3 || (op >= 2 && d.n_extra <= 0)) return hipErrorInvalidValue;
    if (op == 0 || op == 2) scan_solve(s, d.fwd, c.loc_f, d.p, d.t1, c, PgGate{});
    if (op == 1) scan_solve(s, d.bwd, c.loc_b, d.g, d.t2, c, PgGate{});
    if (op == 2) k_pg_extra_u<<<dim3(blocks_for(d.n_extra), c.cols), kPgThreads, 0, s>>>(d, c, d.t1, PgGate{});
    if (op == 3) kt_apply(s, d, c, PgGate{});
    return hipGetLastError();
}

hipError_t pg_async_open(hipStream_t s, const PgDev& d, PgRecord* rec, int max_iterations, double abs_tol, double rel_tol)
{
    if (d.n <= 0) return hipErrorInvalidValue;
    hipError_t e = pg_linearize(s, d, d.X);
    if (e != hipSuccess) return e;
    k_pg_open<<<1, 1, 0, s>>>(d, rec, max_iterations, abs_tol, rel_tol);
    return hipGetLastError();
}

hipError_t pg_async_segment(hipStream_t s, const PgDev& d, PgRecord* rec, double tol, int max_cg, int cg_chunk)
{
    if (d.n <= 0 || cg_chunk <= 0) return hipErrorInvalidValue;
    const PgGate head{ &rec->skip_head, 0 }, tail{ &rec->skip_tail, 0 };
    hipError_t e;
    // head of a step; the CG begin shuts it again
    if ((e = pg_rhs(s, d, head)) || (e = pg_cg_begin(s, d, kPgOne, tol, max_cg, head, &rec->skip_head))) return e;
    if ((e = pg_cg_iterations(s, d, kPgOne, cg_chunk))) return e;
    k_pg_gate<<<1, 1, 0, s>>>(d, rec);
    // tail: the step, the trial point's linearisation, the close
    if ((e = pg_step(s, d, tail)) || (e = pg_linearize(s, d, d.Xtrial, tail))) return e;
    k_pg_close<<<1, 1, 0, s>>>(d, rec);
    k_pg_keep<<<blocks_for(12 * d.n), kPgThreads, 0, s>>>(d, rec);
    return hipGetLastError();
}

hipError_t pg_poses(hipStream_t s, const double* X, int first, int count, float* xyzrpy, float4* pos)
{
    if (count <= 0) return hipSuccess;
    k_pg_poses<<<blocks_for(count), kPgThreads, 0, s>>>(X, first, count, xyzrpy, pos);
    return hipGetLastError();
}

hipError_t pg_store_stage(hipStream_t s, const double* X, int first, int count, float* stage, int32_t* bad)
{
    k_pg_store_stage<<<blocks_for(count), kPgThreads, 0, s>>>(X, first, count, stage, bad);
    return hipGetLastError();
}

hipError_t pg_store_write(hipStream_t s, const float* stage, int count, float4* pos, KfFrame* frames)
{
    k_pg_store_write<<<blocks_for(count), kPgThreads, 0, s>>>(stage, count, pos, frames);
    return hipGetLastError();
}

}  // namespace s2m
