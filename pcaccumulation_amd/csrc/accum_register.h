// C6. Scan-to-map point-to-plane registration against the accumulated scene cloud (accum_register.hip; include/pcacc.h C6):
// the per-point transform and validity, the 27-voxel correspondence search, the 29 terms of a correspondence, the summation order, the 6x6 solve,
// the pose update and the whole round logic as __host__ __device__ functions, so that the SAME code runs in the kernels and in a g++ build
// (tests/accum_register_host_driver.cpp) where every table index is assert-checked before anything runs on a GPU.
// Includes nothing of HIP.  Only +, -, *, / and sqrt in float64 with no FMA contraction, in the order written here: both builds give the same bits.
//
// Per point p of the scan under the current pose T (rows 0-2 of a row-major 4x4):
//   w_a          ((T_a0 x + T_a1 y) + T_a2 z) + T_a3                                       accum_grid.h's transform
//   valid        every w_a finite, |w_a| < 32768, i_a = floor(w_a / voxel_size) in [-2^20, 2^20).  An invalid point has no correspondence: it is never
//                clamped and forms no key.  It still counts in the denominator of the fitness.
//   candidates   every map row with dst[row] >= 0 (extract's filter) whose normal has neither flag 1 nor flag 2, in the 3 x 3 x 3 voxels around
//                (i_x, i_y, i_z), visited in ASCENDING KEY ORDER through accn_column with r = 1 (dx = -1..1, inside it dy = -1..1, inside it the z run);
//                offsets that leave the grid are skipped there before a key is formed.
//   match        the candidate with the smallest d2 = (e_x e_x + e_y e_y) + e_z e_z, e = w - c_j, c_j = accn_centroid (float64); a strict < sends ties
//                to the lowest key; accepted iff d2 <= max_distance^2.  This 27-voxel search IS the contract: no claim about a global nearest neighbour.
//   terms        n = (double)normal32[dst[row]];  r = (n_x e_x + n_y e_y) + n_z e_z;  J = (w x n, n) with w x n = (w_y n_z - w_z n_y, w_z n_x - w_x n_z,
//                w_x n_y - w_y n_x);  t[0..20] = J_a J_b (a <= b, row-major upper triangle), t[21..26] = J_a r, t[27] = r r, t[28] = 1.
//                A point without a correspondence (moving, invalid, nothing within max_distance) has t = +0.0 everywhere.
// Sum of a term over the scan: points are cut into SLOTS of ACCR_SLOT = 256 consecutive points (point i in slot i / 256, position i % 256; positions
// past n hold +0.0).  Inside a slot the 4 groups of 64 consecutive positions each run the tree v[l] += v[l + s] (l < s) for s = 32, 16, 8, 4, 2, 1; the
// slot sum is ((g0 + g1) + g2) + g3; the slots are then added in ascending slot order starting from 0.0.  accr_slot_sum is that order on the host; the
// kernel runs it with wave shuffles.  No floating-point atomics.
// Solve: A = sum J J^T (6x6), b = sum J r.  d_a = sqrt(A_aa); As_ab = A_ab / (d_a d_b), bs_a = b_a / d_a; Cholesky As = L L^T in float64, row by row; a
// diagonal A_aa that is not > 0 or a pivot <= 1e-10 (C3's zero threshold) means a direction nothing constrains (a plane, an edge, too few points):
// DEGENERATE.  Otherwise L y = -bs, L^T z = y, x_a = z_a / d_a, x = (omega, t).
// Update: h = omega / 2; s = sqrt(1 + ((h_x h_x + h_y h_y) + h_z h_z)); q = (1, h) / s (w, x, y, z); R_d = the rotation of the unit quaternion q (no sin /
// cos; a proper rotation to rounding); T <- [R_d | t] T by hd.h's pcacc_pose_compose: N_rc = ((R_r0 T_0c + R_r1 T_1c) + R_r2 T_2c) (+ t_r for c = 3).
// Round k = 0 .. max_iter (accr_round): sums -> correspondences nc, fitness = nc / eligible, rmse = sqrt(sum r^2 / nc); stop when k > 0 and
// |d fitness| < 1e-6 and |d rmse| < 1e-6, or when k = max_iter (status MAX_ITER unless it converged at that very round); else solve and update.
#pragma once
#include "accum_normals.h"

#define ACCR_TERMS 29
#define ACCR_SLOT 256
#define ACCR_GROUP 64
#define ACCR_PIVOT_TOL 1e-10

#define ACCR_NO_ELIGIBLE 1            // every point is flagged moving, or the scan is empty
#define ACCR_NO_CANDIDATE 2           // no map row under the filter has a valid normal
#define ACCR_NO_CORRESPONDENCE 4      // an evaluation found none
#define ACCR_DEGENERATE 8             // the 6x6 system leaves a direction unconstrained
#define ACCR_MAX_ITER 16              // stopped by max_iter, not by the convergence rule
#define ACCR_BAD_TABLE 32             // the normal tables do not have the rows the filter keeps: nothing was addressed

struct AccrState {
    double T[16];                     // the pose so far
    double T_good[16];                // the pose of the last evaluation that had correspondences (the initial pose before any)
    double fit, rmse;                 // of the previous round
    long long eligible, candidates;   // points not flagged moving; map rows with a valid normal under the filter
    int done, iters, status, pad;
};

// World coordinates and voxel of point p under T; false = invalid, w and idx then hold nothing.
PCACC_HD bool accr_world(const double *T, const float *p, double voxel_size, double w[3], int64_t idx[3])
{
    PCACC_NO_CONTRACT
    const double x = p[0], y = p[1], z = p[2];
    for (int a = 0; a < 3; ++a) {
        const double v = ((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3];
        if (!pcacc_finite(v) || !(__builtin_fabs(v) < ACC_COORD_LIMIT)) return false;
        const double c = __builtin_floor(v / voxel_size);
        if (!(c >= -(double)ACC_IDX_BIAS && c < (double)ACC_IDX_BIAS)) return false;
        w[a] = v;
        idx[a] = (int64_t)c;
    }
    return true;
}

// Output row of map row p when it is a candidate, else -1: dst[p] in [0, n_rows) and neither flag 1 nor flag 2 on it.  flags == NULL (C9 only): every
// row the filter keeps is a candidate.
PCACC_HD int64_t accr_candidate(const int *dst, const uint8_t *flags, int64_t n_rows, int64_t p)
{
    const int64_t j = dst[p];
    if (j < 0) return -1;
    if (!flags) return j;                                                                    // register never passes NULL
    if (accn_index(j, n_rows) < 0) return -1;
    return (flags[j] & (ACCN_FEW_NEIGHBORS | ACCN_DEGENERATE)) ? -1 : j;
}

// The correspondence of world point w in voxel idx: its map row (and *out_row = the row of the normal tables, c = its centroid, *out_d2), or -1.
PCACC_HD int64_t accr_match(const unsigned long long *keys, const int64_t *acc, int64_t capacity, int64_t m, const int *dst, const uint8_t *flags,
                            int64_t n_rows, const double w[3], const int64_t idx[3], double max_d2, int64_t *out_row, double c[3], double *out_d2)
{
    PCACC_NO_CONTRACT
    int64_t best = -1, best_row = -1;
    double best_d2 = 0.0;
    if (m > capacity) return -1;
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy) {
            int64_t p0;
            const int n = accn_column(keys, m, idx[0] + dx, idx[1] + dy, idx[2], 1, &p0);
            for (int e = 0; e < n; ++e) {
                const int64_t p = accn_index(p0 + e, m);
                if (p < 0) continue;
                const int64_t j = accr_candidate(dst, flags, n_rows, p);
                if (j < 0) continue;
                const int64_t cnt = acc[accum_field(0, p, capacity)];
                const double cx = accn_centroid(acc[accum_field(2, p, capacity)], cnt), cy = accn_centroid(acc[accum_field(3, p, capacity)], cnt),
                             cz = accn_centroid(acc[accum_field(4, p, capacity)], cnt);
                const double ex = w[0] - cx, ey = w[1] - cy, ez = w[2] - cz;
                const double d2 = (ex * ex + ey * ey) + ez * ez;
                if (best < 0 || d2 < best_d2) {
                    best = p; best_row = j; best_d2 = d2;
                    c[0] = cx; c[1] = cy; c[2] = cz;
                }
            }
        }
    if (best < 0 || !(best_d2 <= max_d2)) return -1;
    *out_row = best_row;
    *out_d2 = best_d2;
    return best;
}

// The 29 terms of a correspondence (world point w, centroid c, float32 normal n32 of the matched row).
PCACC_HD void accr_terms(const double w[3], const double c[3], const float *n32, double t[ACCR_TERMS])
{
    PCACC_NO_CONTRACT
    const double nx = n32[0], ny = n32[1], nz = n32[2];
    const double ex = w[0] - c[0], ey = w[1] - c[1], ez = w[2] - c[2];
    const double r = (nx * ex + ny * ey) + nz * ez;
    double J[6];
    J[0] = w[1] * nz - w[2] * ny;
    J[1] = w[2] * nx - w[0] * nz;
    J[2] = w[0] * ny - w[1] * nx;
    J[3] = nx; J[4] = ny; J[5] = nz;
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) t[k++] = J[a] * J[b];
    for (int a = 0; a < 6; ++a) t[21 + a] = J[a] * r;
    t[27] = r * r;
    t[28] = 1.0;
}

// The 29 terms of scan point i (all +0.0 without a correspondence); *out_map_row = the matched map row or -1.
PCACC_HD void accr_point(const unsigned long long *keys, const int64_t *acc, int64_t capacity, int64_t m, const int *dst, const float *normals,
                         const uint8_t *flags, int64_t n_rows, const double *T, const float *points, const uint8_t *moving, int64_t n, int64_t i,
                         double voxel_size, double max_d2, double t[ACCR_TERMS], int64_t *out_map_row)
{
    for (int k = 0; k < ACCR_TERMS; ++k) t[k] = 0.0;
    *out_map_row = -1;
    if (accn_index(i, n) < 0) return;
    if (moving && moving[i]) return;
    double w[3], c[3], d2;
    int64_t idx[3], row;
    if (!accr_world(T, points + 3 * i, voxel_size, w, idx)) return;
    const int64_t p = accr_match(keys, acc, capacity, m, dst, flags, n_rows, w, idx, max_d2, &row, c, &d2);
    if (p < 0) return;
    accr_terms(w, c, normals + 3 * row, t);
    *out_map_row = p;
}

// The sum of one term over a slot: v[ACCR_SLOT] is used as scratch.
PCACC_HD double accr_slot_sum(double *v)
{
    PCACC_NO_CONTRACT
    for (int g = 0; g < ACCR_SLOT / ACCR_GROUP; ++g)
        for (int s = ACCR_GROUP / 2; s > 0; s >>= 1)
            for (int l = 0; l < s; ++l) v[g * ACCR_GROUP + l] = v[g * ACCR_GROUP + l] + v[g * ACCR_GROUP + l + s];
    double sum = v[0];
    for (int g = 1; g < ACCR_SLOT / ACCR_GROUP; ++g) sum = sum + v[g * ACCR_GROUP];
    return sum;
}

// x = (omega, t) of the summed terms; false = DEGENERATE (x then holds nothing).
PCACC_HD bool accr_solve(const double s[ACCR_TERMS], double x[6])
{
    PCACC_NO_CONTRACT
    double A[6][6], L[6][6], d[6], y[6];
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) { A[a][b] = s[k]; A[b][a] = s[k]; ++k; }
    for (int a = 0; a < 6; ++a) {
        if (!(A[a][a] > 0.0) || !pcacc_finite(A[a][a])) return false;
        d[a] = __builtin_sqrt(A[a][a]);
    }
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) A[a][b] = A[a][b] / (d[a] * d[b]);
    for (int a = 0; a < 6; ++a) {
        for (int b = 0; b < a; ++b) {
            double v = A[a][b];
            for (int c = 0; c < b; ++c) v = v - L[a][c] * L[b][c];
            L[a][b] = v / L[b][b];
        }
        double piv = A[a][a];
        for (int c = 0; c < a; ++c) piv = piv - L[a][c] * L[a][c];
        if (!(piv > ACCR_PIVOT_TOL)) return false;
        L[a][a] = __builtin_sqrt(piv);
    }
    for (int a = 0; a < 6; ++a) {
        double v = 0.0 - s[21 + a] / d[a];
        for (int c = 0; c < a; ++c) v = v - L[a][c] * y[c];
        y[a] = v / L[a][a];
    }
    for (int a = 5; a >= 0; --a) {
        double v = y[a];
        for (int c = a + 1; c < 6; ++c) v = v - L[c][a] * x[c];
        x[a] = v / L[a][a];
    }
    for (int a = 0; a < 6; ++a) {
        x[a] = x[a] / d[a];
        if (!pcacc_finite(x[a])) return false;
    }
    return true;
}

// T <- [R_d | t] T for x = (omega, t); rows 0-2 of T.
PCACC_HD void accr_compose(const double x[6], double *T)
{
    PCACC_NO_CONTRACT
    const double hx = x[0] / 2.0, hy = x[1] / 2.0, hz = x[2] / 2.0;
    const double s = __builtin_sqrt(1.0 + ((hx * hx + hy * hy) + hz * hz));
    const double qw = 1.0 / s, qx = hx / s, qy = hy / s, qz = hz / s;
    double R[9];
    R[0] = 1.0 - 2.0 * (qy * qy + qz * qz); R[1] = 2.0 * (qx * qy - qw * qz); R[2] = 2.0 * (qx * qz + qw * qy);
    R[3] = 2.0 * (qx * qy + qw * qz); R[4] = 1.0 - 2.0 * (qx * qx + qz * qz); R[5] = 2.0 * (qy * qz - qw * qx);
    R[6] = 2.0 * (qx * qz - qw * qy); R[7] = 2.0 * (qy * qz + qw * qx); R[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
    pcacc_pose_compose(R, x + 3, T);
}

// A fresh job: the pose is rows 0-2 of init (NULL = identity), row 3 is 0 0 0 1.
PCACC_HD void accr_init(AccrState *st, const double *init, int64_t eligible, int64_t candidates)
{
    pcacc_pose_seed(st->T, init);
    for (int k = 0; k < 16; ++k) st->T_good[k] = st->T[k];
    st->fit = st->rmse = 0.0;
    st->eligible = eligible;
    st->candidates = candidates;
    st->done = st->iters = st->status = st->pad = 0;
}

struct AccrOut {                      // written once, by the round that finishes the job
    double *pose, *fitness, *rmse;    // [16], [1], [1]
    int32_t *iterations, *status, *correspondences;
};

PCACC_HD void accr_finish(AccrState *st, const AccrOut *o, const double *pose, double fit, double rmse, int iters, int status, double nc)
{
    for (int k = 0; k < 16; ++k) o->pose[k] = pose[k];
    *o->fitness = fit;
    *o->rmse = rmse;
    *o->iterations = iters;
    *o->status = status;
    *o->correspondences = (int32_t)nc;
    st->status = status;
    st->iters = iters;
    st->done = 1;
}

// Round `round` of a job that is not done, from the summed terms of the evaluation under st->T.
PCACC_HD void accr_round(AccrState *st, const double s[ACCR_TERMS], int round, int max_iter, const AccrOut *o)
{
    PCACC_NO_CONTRACT
    if (st->status & ACCR_BAD_TABLE) { accr_finish(st, o, st->T_good, 0.0, 0.0, 0, ACCR_BAD_TABLE, 0.0); return; }
    if (st->eligible <= 0 || st->candidates <= 0) {
        accr_finish(st, o, st->T_good, 0.0, 0.0, st->iters,
                    st->status | (st->eligible <= 0 ? ACCR_NO_ELIGIBLE : 0) | (st->candidates <= 0 ? ACCR_NO_CANDIDATE : 0), 0.0);
        return;
    }
    const double nc = s[28];
    if (!(nc > 0.0)) { accr_finish(st, o, st->T_good, 0.0, 0.0, st->iters, st->status | ACCR_NO_CORRESPONDENCE, 0.0); return; }
    const double fit = nc / (double)st->eligible;
    const double rmse = __builtin_sqrt(s[27] / nc);
    for (int k = 0; k < 16; ++k) st->T_good[k] = st->T[k];
    const bool converged = round > 0 && pcacc_icp_stop(fit, st->fit, rmse, st->rmse);
    if (converged || round >= max_iter) {
        accr_finish(st, o, st->T, fit, rmse, round, st->status | (converged ? 0 : ACCR_MAX_ITER), nc);
        return;
    }
    double x[6];
    if (!accr_solve(s, x)) { accr_finish(st, o, st->T, 0.0, 0.0, round, st->status | ACCR_DEGENERATE, nc); return; }
    accr_compose(x, st->T);
    st->fit = fit;
    st->rmse = rmse;
    st->iters = round + 1;
}
