// s2m_icp_close.hpp — what closes one ICP iteration, once the 17 sums of its correspondences are known: Eigen::umeyama without
// scaling (the fp64 one-sided Jacobi SVD behind it), the float composition into the running transformation and PCL's convergence
// state machine (PCL 1.10 [ext]: registration/impl/icp.hpp computeTransformation, default_convergence_criteria.hpp hasConverged).
// ONE source for the host loop of icp_align and for the device loop's k_icp_close (s2m_icp.hip): every function here is
// __host__ __device__, the library is built with -ffp-contract=off for both sides, and the two fp64 operations whose rounding
// a device library could choose (sqrt, divide) go through icp_sqrt / icp_div, the correctly rounded forms on the device. So
// both loops produce the same bits from the same sums.  Includes nothing but <cmath>: a host compiler builds it stand-alone.
#pragma once
#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define S2M_ICP_HD __host__ __device__
#else
#define S2M_ICP_HD
#endif

namespace s2m {

S2M_ICP_HD inline double icp_sqrt(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(x);
#else
    return std::sqrt(x);
#endif
}

S2M_ICP_HD inline double icp_div(double a, double b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}

S2M_ICP_HD inline double icp_fabs(double x) { return x < 0.0 ? -x : (x == 0.0 ? 0.0 : x); }   // fabs: -0.0 -> +0.0, NaN stays NaN

S2M_ICP_HD inline void icp_swap(double& a, double& b) { const double t = a; a = b; b = t; }

// Eigen::umeyama without scaling, as pcl::registration::TransformationEstimationSVD uses it (reference
// src/mapOptmization.cpp:583 -> icp.align, PCL 1.10 [ext]): R = U S V^T of the cross-covariance sigma =
// (1/n) sum (tgt - mean_tgt)(src - mean_src)^T with S(2) = -1 if det(U) det(V) < 0, t = mean_tgt - R mean_src.
// The 3x3 SVD is a one-sided Jacobi in fp64 (Eigen: JacobiSVD<Matrix3f>); T is row-major 4x4.
S2M_ICP_HD inline void host_svd3(const double A[9], double U[9], double S[3], double V[9])
{
    double W[9];
    for (int i = 0; i < 9; i++) { W[i] = A[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0.0;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double a = 0, b = 0, c = 0;
                for (int k = 0; k < 3; k++) { a += W[k * 3 + p] * W[k * 3 + p]; b += W[k * 3 + q] * W[k * 3 + q]; c += W[k * 3 + p] * W[k * 3 + q]; }
                off += c * c;
                if (icp_fabs(c) <= 1e-300 || icp_fabs(c) <= 1e-17 * icp_sqrt(a * b)) continue;
                const double zeta = icp_div(b - a, 2.0 * c);
                const double t = icp_div(zeta >= 0 ? 1.0 : -1.0, icp_fabs(zeta) + icp_sqrt(1.0 + zeta * zeta));
                const double cs = icp_div(1.0, icp_sqrt(1.0 + t * t)), sn = cs * t;
                for (int k = 0; k < 3; k++) {
                    const double wp = W[k * 3 + p], wq = W[k * 3 + q];
                    W[k * 3 + p] = cs * wp - sn * wq; W[k * 3 + q] = sn * wp + cs * wq;
                    const double vp = V[k * 3 + p], vq = V[k * 3 + q];
                    V[k * 3 + p] = cs * vp - sn * vq; V[k * 3 + q] = sn * vp + cs * vq;
                }
            }
        if (off < 1e-300) break;
    }
    for (int j = 0; j < 3; j++) {
        double nrm = 0;
        for (int k = 0; k < 3; k++) nrm += W[k * 3 + j] * W[k * 3 + j];
        S[j] = icp_sqrt(nrm);
    }
    for (int i = 0; i < 2; i++)
        for (int j = i + 1; j < 3; j++)
            if (S[j] > S[i]) {
                icp_swap(S[i], S[j]);
                for (int k = 0; k < 3; k++) { icp_swap(W[k * 3 + i], W[k * 3 + j]); icp_swap(V[k * 3 + i], V[k * 3 + j]); }
            }
    for (int j = 0; j < 3; j++)
        for (int k = 0; k < 3; k++) U[k * 3 + j] = S[j] > 1e-300 ? icp_div(W[k * 3 + j], S[j]) : 0.0;
    // U is orthonormal for every input, as Eigen's JacobiSVD returns it. Rank 0 (A = 0: no rotation ran, V = I): U = I.
    if (!(S[0] > 1e-300)) { for (int i = 0; i < 9; i++) U[i] = (i % 4 == 0) ? 1.0 : 0.0; return; }
    // Rank 1 (column 1 of W is zero, or what the rotations left of a zero: W[., 1] / S[1] would be column 0 again): column 1 is
    // column 0 crossed with the axis of its smallest |component| (the first of equals), normalised; column 2 follows below.
    if (S[1] <= 1e-12 * S[0]) {
        const double u0 = U[0], u1 = U[3], u2 = U[6];
        int ax = 0;
        if (icp_fabs(u1) < icp_fabs(u0)) ax = 1;
        if (icp_fabs(u2) < icp_fabs(ax == 0 ? u0 : u1)) ax = 2;
        const double c0 = ax == 0 ? 0.0 : (ax == 1 ? -u2 : u1);          // (u0, u1, u2) x e_ax
        const double c1 = ax == 0 ? u2 : (ax == 1 ? 0.0 : -u0);
        const double c2 = ax == 0 ? -u1 : (ax == 1 ? u0 : 0.0);
        const double nrm = icp_sqrt((c0 * c0 + c1 * c1) + c2 * c2);
        U[1] = icp_div(c0, nrm); U[4] = icp_div(c1, nrm); U[7] = icp_div(c2, nrm);
    }
    if (S[2] <= 1e-12 * S[0]) {          // rank-deficient: complete U to an orthonormal basis
        U[2] = U[3] * U[7] - U[6] * U[4]; U[5] = U[6] * U[1] - U[0] * U[7]; U[8] = U[0] * U[4] - U[3] * U[1];
    }
}

S2M_ICP_HD inline double host_det3(const double M[9])
{
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

S2M_ICP_HD inline void host_umeyama(const float mean_src[3], const float mean_tgt[3], const float sigma[9], float T[16])
{
    double A[9], U[9], S[3], V[9];
    for (int i = 0; i < 9; i++) A[i] = (double)sigma[i];
    host_svd3(A, U, S, V);
    const double sgn[3] = { 1.0, 1.0, (host_det3(U) * host_det3(V) < 0) ? -1.0 : 1.0 };
    float R[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double a = 0;
            for (int k = 0; k < 3; k++) a += U[i * 3 + k] * sgn[k] * V[j * 3 + k];
            R[i * 3 + j] = (float)a;
        }
    for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T[i * 4 + j] = R[i * 3 + j];
        T[i * 4 + 3] = mean_tgt[i] - (R[i * 3 + 0] * mean_src[0] + R[i * 3 + 1] * mean_src[1] + R[i * 3 + 2] * mean_src[2]);
    }
}

// The state an alignment carries from iteration to iteration. On the device it is the head of the loop's state block.
struct IcpLoopState {
    float  T[16];          // final_transformation_ so far (row-major 4x4)
    float  T_step[16];     // transformation_ of the iteration closed last: what k_icp_transform applies to the source
    double prev_mse;       // correspondences_prev_mse_
    int    it;             // nr_iterations_
    int    conv;           // hasConverged()
    int    similar;        // iterations_similar_transforms_
    int    done;           // the alignment has ended: every later kernel of the iteration loop returns at entry
};

// setMaximumIterations, and the thresholds default_convergence_criteria.hpp derives from setTransformationEpsilon /
// setEuclideanFitnessEpsilon (rotation threshold 1 - eps, translation threshold eps, absolute MSE 1e-12, relative MSE)
struct IcpCloseParams { int max_iter; double rot_thr, trl_thr, mse_abs, mse_rel; int max_similar; };

S2M_ICP_HD inline IcpCloseParams icp_close_params(int max_iter, double trans_eps, double fit_eps)
{
    return IcpCloseParams{ max_iter, 1.0 - trans_eps, trans_eps, 1e-12, fit_eps, 0 /* max_iterations_similar_transforms_ */ };
}

// guess: final_transformation_ at the start (align(output, guess)), a row-major 4x4; null: the identity
S2M_ICP_HD inline void icp_state_init(IcpLoopState* st, const float* guess = nullptr)
{
    for (int i = 0; i < 16; i++) { st->T_step[i] = (i % 5 == 0) ? 1.0f : 0.0f; st->T[i] = guess ? guess[i] : st->T_step[i]; }
    st->prev_mse = DBL_MAX;
    st->it = 0; st->conv = 0; st->similar = 0; st->done = 0;
}

// One iteration's close on its sums S = {count, sum d2, sum src (3), sum tgt (3), sum tgt src^T (9)}: icp.hpp
// computeTransformation's loop body behind determineCorrespondences + default_convergence_criteria.hpp hasConverged.
// Sets st->done when the alignment ends; T_step is written unless it ends on too few correspondences.
S2M_ICP_HD inline void icp_close_step(const double S[17], const IcpCloseParams& p, IcpLoopState* st)
{
    const double cnt = S[0];
    if (cnt < 3.0) { st->conv = 0; st->done = 1; return; }                // min_number_correspondences_
    const double mse = icp_div(S[1], cnt);
    float ms[3], mt[3], sg[9];
    for (int d = 0; d < 3; d++) { ms[d] = (float)icp_div(S[2 + d], cnt); mt[d] = (float)icp_div(S[5 + d], cnt); }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) sg[r * 3 + c] = (float)(icp_div(S[8 + r * 3 + c], cnt) - icp_div(S[5 + r], cnt) * icp_div(S[2 + c], cnt));
    float* T = st->T_step;
    host_umeyama(ms, mt, sg, T);
    float F[16];
    for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) {
            float a = 0;
            for (int k = 0; k < 4; k++) a += T[r * 4 + k] * st->T[k * 4 + c];
            F[r * 4 + c] = a;
        }
    for (int i = 0; i < 16; i++) st->T[i] = F[i];
    ++st->it;
    int is_similar = 0;
    if (st->it >= p.max_iter) { st->conv = 1; st->done = 1; return; }     // CONVERGENCE_CRITERIA_ITERATIONS
    const double cos_angle = 0.5 * ((double)T[0] + (double)T[5] + (double)T[10] - 1.0);
    const double tsq = (double)T[3] * T[3] + (double)T[7] * T[7] + (double)T[11] * T[11];
    if (cos_angle >= p.rot_thr && tsq <= p.trl_thr) { if (st->similar >= p.max_similar) { st->conv = 1; st->done = 1; return; } is_similar = 1; }
    if (icp_fabs(mse - st->prev_mse) < p.mse_abs) { if (st->similar >= p.max_similar) { st->conv = 1; st->done = 1; return; } is_similar = 1; }
    if (icp_div(icp_fabs(mse - st->prev_mse), st->prev_mse) < p.mse_rel) { if (st->similar >= p.max_similar) { st->conv = 1; st->done = 1; return; } is_similar = 1; }
    st->similar = is_similar ? st->similar + 1 : 0;
    st->prev_mse = mse;
}

}  // namespace s2m
