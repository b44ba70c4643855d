// C3. One round of the ICP refinement (icp.hip): the partition of a job's source into slices, the 17 terms of a correspondence, their summation
// order, the statistics, the stop rule, the status bits, the Umeyama update on svd3.h's SVD and the pose composition as __host__ __device__
// functions, so that the SAME code runs in the kernels and in a g++ build (tests/icp_host_driver.cpp) which runs the whole loop with every table
// index assert-checked before anything runs on a GPU.  Includes nothing of HIP.  Only +, -, *, / and sqrt in float64 with no FMA contraction, in the
// order written here: both builds give the same bits.
//
// Slices: every job's source segment [lo, hi) is cut into `slices` = icp_slices(n, n_jobs) pieces of per = ceil((hi - lo) / slices) consecutive
// points; slice k is [lo + k per, min(lo + (k + 1) per, hi)), empty when it starts at or behind hi.
// Terms of a correspondence (q = the source point under the current pose, t = its target, d2 their squared distance):
//   [0] 1   [1..3] q   [4..6] t   [7 + 3 c + d] t_c * q_d   [16] d2.     A point without a correspondence adds nothing.
// Sum of a term over a slice [a, b): lane l of ICP_BLOCK = 256 adds the points a + l, a + l + 256, ... in that order starting from 0.0
// (icp_lane_sums); then the tree v[l] += v[l + s] (l < s) for s = 128, 64, .. 1 over the 256 lane values (icp_tree_sum); the slice sum is v[0].
// The slices of a job are then added in ascending slice order starting from 0.0.  icp_slice_sums is the first two steps on the host; the kernel
// runs icp_lane_sums on every lane and the tree in LDS.  No floating-point atomics.
// Round k = 0 .. max_iter (icp_round), from the sums of the evaluation under st->T: nc = sums[0], fitness = nc / source points, rmse =
// sqrt(sums[16] / nc) (0 without correspondences); stop when k > 0 and hd.h's pcacc_icp_stop holds against the previous round, or when
// k = max_iter.  Otherwise, with correspondences: ms = sum q / nc, mt = sum t / nc, cov_cd = sum t_c q_d / nc - mt_c ms_d; u s v^T =
// jacobi_svd3_floor(cov, noise) with noise = 1e-10 * (|S_00| + |S_11| + |S_22|) / nc, the rounding of the uncentred sums: a covariance that is zero in
// exact arithmetic -- every source matched to ONE target -- gives the identity and not a rotation read out of rounding errors;
// R_rc = (u_r0 v_c0 + u_r1 v_c1) + (g u_r2) v_c2 with g = -1 when det(u) det(v) < 0 (Umeyama's reflection fix), else +1; t = mt - R ms;
// T <- [R | t] T by pcacc_pose_compose.  Rank < 3 sets PCACC_ICP_RANK_DEFICIENT (svd3.h completes the basis: a proper rotation, the same every run);
// rank 0, or an R that is not finite, gives the identity rotation.
#pragma once
#include "../../include/pcacc.h"          // the PCACC_ICP_* status bits: plain C
#include "icp_grid.h"
#include "svd3.h"

#define ICP_BLOCK 256
#define ICP_SUMS 17
#define ICP_MAX_SLICES 64

struct IcpState {                     // per job, in the workspace
    double T[16];                     // accumulated update @ initial pose
    double fit, rmse;                 // of the previous round
    int32_t done, iters, status, pad;
};

struct IcpOut {                       // of one job; written once, by the round that finishes it
    double *pose, *fitness, *rmse;    // [16], [1], [1]
    int32_t *iterations, *status;
};

// Slices of a job's source: enough workgroups to fill the device when there are few jobs, never more than 256-point pieces of the whole array.
PCACC_HD int icp_slices(int64_t n, int32_t n_jobs)
{
    int slices = n_jobs > 0 ? 2048 / n_jobs : 1;
    const int64_t pieces = (n + ICP_BLOCK - 1) / ICP_BLOCK;
    if (slices > ICP_MAX_SLICES) slices = ICP_MAX_SLICES;
    if (slices > pieces) slices = (int)pieces;
    if (slices < 1) slices = 1;
    return slices;
}

PCACC_HD void icp_slice_bounds(int64_t lo, int64_t hi, int slices, int slice, int64_t *a, int64_t *b)
{
    const int64_t per = (hi - lo + slices - 1) / slices;
    *a = lo + slice * per;
    *b = *a + per < hi ? *a + per : hi;
}

PCACC_HD void icp_terms(const double q[3], const double t[3], double d2, double term[ICP_SUMS])
{
    PCACC_NO_CONTRACT
    term[0] = 1.0;
    for (int c = 0; c < 3; ++c) {
        term[1 + c] = q[c];
        term[4 + c] = t[c];
        for (int d = 0; d < 3; ++d) term[7 + 3 * c + d] = t[c] * q[d];
    }
    term[16] = d2;
}

// What lane `lane` of the workgroup of slice [a, b) adds up: acc [ICP_SUMS].  T: rows 0-2 of the job's pose; tgt: its target segment.
PCACC_HD void icp_lane_sums(const IcpGrid &g, int tgt, const double *T, double thr2, int64_t a, int64_t b, int lane, double *acc)
{
    PCACC_NO_CONTRACT
    for (int k = 0; k < ICP_SUMS; ++k) acc[k] = 0.0;
    for (int64_t i = a + lane; i < b; i += ICP_BLOCK) {
        PCACC_BOUND(i, g.n);
        double q[3], d2, term[ICP_SUMS];
        icp_apply(T, g.points + 3 * i, q);
        const int64_t m = icp_nearest(g, tgt, q, thr2, &d2);
        if (m < 0) continue;
        const double t[3] = {(double)g.points[3 * m], (double)g.points[3 * m + 1], (double)g.points[3 * m + 2]};
        icp_terms(q, t, d2, term);
        for (int k = 0; k < ICP_SUMS; ++k) acc[k] = acc[k] + term[k];
    }
}

// The tree over the ICP_BLOCK lane values of one term; v is used as scratch.
PCACC_HD double icp_tree_sum(double *v)
{
    PCACC_NO_CONTRACT
    for (int s = ICP_BLOCK / 2; s > 0; s >>= 1)
        for (int l = 0; l < s; ++l) v[l] = v[l] + v[l + s];
    return v[0];
}

// The 17 sums of slice [a, b) in the kernel's order, on the host.
PCACC_HD void icp_slice_sums(const IcpGrid &g, int tgt, const double *T, double thr2, int64_t a, int64_t b, double sums[ICP_SUMS])
{
    double v[ICP_SUMS][ICP_BLOCK], acc[ICP_SUMS];
    for (int lane = 0; lane < ICP_BLOCK; ++lane) {
        icp_lane_sums(g, tgt, T, thr2, a, b, lane, acc);
        for (int k = 0; k < ICP_SUMS; ++k) v[k][lane] = acc[k];
    }
    for (int k = 0; k < ICP_SUMS; ++k) sums[k] = icp_tree_sum(v[k]);
}

// The least-squares rotation of a covariance; false = rank-deficient (the rotation is then one valid choice, or the identity at rank 0).
PCACC_HD bool icp_kabsch_rotation(const double cov[3][3], double noise, double R[9])
{
    PCACC_NO_CONTRACT
    double u[3][3], s[3], v[3][3];
    const int rank = jacobi_svd3_floor(cov, noise, u, s, v);
    auto det = [](const double m[3][3]) {
        return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
               m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
    };
    const double g = det(u) * det(v) < 0.0 ? -1.0 : 1.0;
    bool finite = rank > 0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            R[3 * r + c] = (u[r][0] * v[c][0] + u[r][1] * v[c][1]) + (g * u[r][2]) * v[c][2];
            if (!pcacc_finite(R[3 * r + c])) finite = false;
        }
    if (!finite)
        for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    return finite && rank == 3;
}

// Round `round` of a job that is not done, from the summed terms of the evaluation under st->T.  n_src, n_tgt: points of its two segments.
PCACC_HD void icp_round(IcpState *st, const double sums[ICP_SUMS], int64_t n_src, int64_t n_tgt, int round, int max_iter, const IcpOut *o)
{
    PCACC_NO_CONTRACT
    const double nc = sums[0];
    const double fit = n_src > 0 ? nc / (double)n_src : 0.0;
    const double rmse = nc > 0.0 ? __builtin_sqrt(sums[16] / nc) : 0.0;
    int status = st->status | (n_src == 0 ? PCACC_ICP_EMPTY_SOURCE : 0) | (n_tgt == 0 ? PCACC_ICP_EMPTY_TARGET : 0);
    const bool converged = round > 0 && pcacc_icp_stop(fit, st->fit, rmse, st->rmse);
    if (converged || round >= max_iter) {
        if (!(nc > 0.0)) status |= PCACC_ICP_NO_CORRESPONDENCE;
        for (int k = 0; k < 16; ++k) o->pose[k] = st->T[k];
        *o->fitness = fit;
        *o->rmse = rmse;
        *o->iterations = round;
        *o->status = status;
        st->status = status;
        st->done = 1;
        return;
    }
    if (nc > 0.0) {                                                         // no correspondences: the update is the identity
        double ms[3], mt[3], cov[3][3], R[9], t[3];
        for (int c = 0; c < 3; ++c) { ms[c] = sums[1 + c] / nc; mt[c] = sums[4 + c] / nc; }
        for (int c = 0; c < 3; ++c)
            for (int d = 0; d < 3; ++d) cov[c][d] = sums[7 + 3 * c + d] / nc - mt[c] * ms[d];
        // 1e-10 of the mean of t . q: far above the rounding of the sums (2^-53 times at most the number of terms), far below the covariance of
        // any cloud that has an extent (a singular value of 1e-10 of the squared distance from the origin is a thickness of micrometres)
        const double noise = 1e-10 * (__builtin_fabs(sums[7]) + __builtin_fabs(sums[11]) + __builtin_fabs(sums[15])) / nc;
        if (!icp_kabsch_rotation(cov, noise, R)) status |= PCACC_ICP_RANK_DEFICIENT;
        for (int c = 0; c < 3; ++c) t[c] = mt[c] - (R[3 * c] * ms[0] + R[3 * c + 1] * ms[1] + R[3 * c + 2] * ms[2]);
        pcacc_pose_compose(R, t, st->T);
    }
    st->fit = fit;
    st->rmse = rmse;
    st->iters = round + 1;
    st->status = status;
}
