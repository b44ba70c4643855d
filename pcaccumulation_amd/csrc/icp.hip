// C3. Point-to-point ICP of J independent (source segment, target segment) jobs -- the test-time pose refinement of models/egomotion.py:9-28,
// :360-384 (model.ego_icp) and models/alignnet.py:54-112 (model.tpointnet_icp), which the reference runs through Open3D's registration_icp on
// the host, one call per frame and per instance.  include/pcacc.h (C3) has the contract; DESIGN.md section 9b the argument.
//
//   icp_setup    validates the segment and job tables (a bad table stops every later kernel: nothing is addressed through it), marks the target
//                segments, seeds every job's pose with its initial pose.
//   icp_insert   every finite, in-range point of a target segment claims the hash slot of its (segment, cell) key with one 64-bit CAS and
//                counts itself there; icp_fill (behind a scan of the counts: scan.h) writes the point lists.  The index is built ONCE per call:
//                the target of a job is fixed over all rounds, and the T - 1 jobs of a sample share one target segment.
//   icp_corr     round r, workgroup (job, slice): the slice's source points under the job's current pose, nearest target through the 27-cell
//                walk of icp_grid.h, 17 float64 sums (count, sum q, sum t, sum t q^T, sum d^2) reduced in a fixed order into the slot of (job, slice).
//   icp_update   round r, one wave per job: the slots added in slice order, fitness / rmse, the convergence test against the previous round,
//                then the least-squares rigid update (Umeyama without scale, 3x3 one-sided Jacobi SVD) composed onto the pose.
// All arithmetic on coordinates is float64.  No floating-point atomics, no order that depends on scheduling: the order of the entries in a cell's
// list does (integer atomics), but the walk picks by (distance^2, index), so two runs give the same bits.  Convergence is per job on the device;
// a finished job's later rounds return at once; the host never waits inside the loop (2 * (max_iter + 1) launches, queued back to back).
#include "common.h"
#include "icp_grid.h"
#include "scan.h"

#define ICP_BLOCK 256
#define ICP_SUMS 17
#define ICP_MAX_SLICES 64
#define ICP_BAD_TABLE 1            // ctrl[0]

struct IcpState {                  // per job, in the workspace
    double T[16];                  // accumulated update @ initial pose
    double fit, rmse;              // of the previous round
    int32_t done, iters, status, pad;
};

struct IcpWs {
    unsigned long long *keys;      // [slots]      | zero-filled per call
    int32_t *cnt;                  // [slots]      | counts, then (cleared by the scan) the fill cursors
    int32_t *tflag;                // [n_seg]      | 1 = some job's target
    int32_t *ctrl;                 // [16]         | [0] ICP_BAD_TABLE
    size_t zero_bytes;
    int32_t *start;                // [slots + 1]
    int32_t *pslot;                // [n] slot of a stored target point, -1 otherwise
    int32_t *list;                 // [n]
    int32_t *sums;                 // [chunks of slots + 1]
    double *partial;               // [J][slices][ICP_SUMS]
    IcpState *state;               // [J]
    uint32_t slots;
    int slices;
};

static bool icp_sizes_ok(int64_t n, int32_t n_seg, int32_t n_jobs, int32_t max_iter)
{
    return n >= 0 && n <= (1ll << 29) && n_seg >= 1 && n_seg <= ICP_MAX_SEGMENTS && n_jobs >= 0 && n_jobs <= (1 << 20) && max_iter >= 0 &&
           max_iter <= 10000;
}

static size_t icp_carve(IcpWs *w, char *base, int64_t n, int32_t n_seg, int32_t n_jobs)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += pcacc_align(bytes); return p; };
    uint32_t slots = 64;
    while ((int64_t)slots < 2 * n) slots <<= 1;
    w->slots = slots;
    // slices of a job's source: enough workgroups to fill the device when there are few jobs, never more than 256-point pieces of the whole array
    int slices = n_jobs > 0 ? 2048 / n_jobs : 1;
    const int64_t pieces = (n + ICP_BLOCK - 1) / ICP_BLOCK;
    if (slices > ICP_MAX_SLICES) slices = ICP_MAX_SLICES;
    if (slices > pieces) slices = (int)pieces;
    if (slices < 1) slices = 1;
    w->slices = slices;
    w->keys = (unsigned long long *)take((size_t)slots * 8);
    w->cnt = (int32_t *)take((size_t)slots * 4);
    w->tflag = (int32_t *)take((size_t)n_seg * 4);
    w->ctrl = (int32_t *)take(16 * 4);
    w->zero_bytes = off;
    w->start = (int32_t *)take(((size_t)slots + 1) * 4);
    w->pslot = (int32_t *)take((size_t)(n > 0 ? n : 1) * 4);
    w->list = (int32_t *)take((size_t)(n > 0 ? n : 1) * 4);
    w->sums = (int32_t *)take(((size_t)pcacc_chunks(slots) + 1) * 4);
    w->partial = (double *)take((size_t)(n_jobs > 0 ? n_jobs : 1) * slices * ICP_SUMS * 8);
    w->state = (IcpState *)take((size_t)(n_jobs > 0 ? n_jobs : 1) * sizeof(IcpState));
    return off;
}

extern "C" int pcacc_icp_point_to_point_workspace_bytes(int64_t n, int32_t n_seg, int32_t n_jobs, size_t *bytes)
{
    if (!bytes || !icp_sizes_ok(n, n_seg, n_jobs, 0)) return PCACC_E_ARG;
    IcpWs w;
    *bytes = icp_carve(&w, nullptr, n, n_seg, n_jobs);
    return 0;
}

__global__ __launch_bounds__(ICP_BLOCK) void icp_setup(const int32_t *__restrict__ offsets, int n_seg, const int32_t *__restrict__ jobs, int n_jobs,
                                                       int64_t n, const double *__restrict__ init, IcpWs w)
{
    const int i = blockIdx.x * ICP_BLOCK + threadIdx.x;
    if (i <= n_seg) {
        const int64_t a = offsets[i];
        bool bad = a < 0 || a > n;
        if (i < n_seg && a > (int64_t)offsets[i + 1]) bad = true;
        if (bad) atomicOr(&w.ctrl[0], ICP_BAD_TABLE);
    }
    if (i < n_jobs) {
        const int src = jobs[2 * i], tgt = jobs[2 * i + 1];
        IcpState &s = w.state[i];
        if (src < 0 || src >= n_seg || tgt < 0 || tgt >= n_seg) atomicOr(&w.ctrl[0], ICP_BAD_TABLE);
        else w.tflag[tgt] = 1;
        for (int k = 0; k < 12; ++k) s.T[k] = init ? init[16 * (int64_t)i + k] : ((k % 5 == 0) ? 1.0 : 0.0);
        s.T[12] = s.T[13] = s.T[14] = 0.0;
        s.T[15] = 1.0;
        s.fit = s.rmse = 0.0;
        s.done = s.iters = s.status = s.pad = 0;
    }
}

__global__ __launch_bounds__(ICP_BLOCK) void icp_insert(const float *__restrict__ points, int64_t n, const int32_t *__restrict__ offsets, int n_seg,
                                                        double h, IcpWs w)
{
    if (w.ctrl[0] != 0) return;
    const uint32_t mask = w.slots - 1;
    for (int64_t i = (int64_t)blockIdx.x * ICP_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * ICP_BLOCK) {
        int slot = -1;
        const int seg = icp_segment_of(offsets, n_seg, i);
        if (seg >= 0 && w.tflag[seg]) {
            const double p[3] = {(double)points[3 * i], (double)points[3 * i + 1], (double)points[3 * i + 2]};
            int c[3];
            if (icp_target_cell(p, h, c)) {
                const unsigned long long key = icp_key(seg, c[0], c[1], c[2]);
                uint32_t s = icp_hash(key, mask);
                for (uint32_t probes = 0; probes <= mask; ++probes, s = (s + 1) & mask) {     // slots >= 2 n: an empty slot always exists
                    const unsigned long long k = atomicCAS(&w.keys[s], 0ull, key);
                    if (k == 0 || k == key) { slot = (int)s; break; }
                }
                if (slot >= 0) atomicAdd(&w.cnt[slot], 1);
            }
        }
        w.pslot[i] = slot;
    }
}

__global__ __launch_bounds__(ICP_BLOCK) void icp_fill(int64_t n, IcpWs w)
{
    if (w.ctrl[0] != 0) return;
    for (int64_t i = (int64_t)blockIdx.x * ICP_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * ICP_BLOCK) {
        const int s = w.pslot[i];
        if (s < 0) continue;
        const int64_t e = (int64_t)w.start[s] + atomicAdd(&w.cnt[s], 1);
        if (e >= 0 && e < n) w.list[e] = (int32_t)i;                        // e < start[s + 1] <= stored points <= n by construction
    }
}

__global__ __launch_bounds__(ICP_BLOCK) void icp_corr(const float *__restrict__ points, int64_t n, const int32_t *__restrict__ offsets,
                                                      const int32_t *__restrict__ jobs, double h, double thr2, IcpWs w)
{
    __shared__ double red[ICP_SUMS][ICP_BLOCK];
    const int j = blockIdx.x, slice = blockIdx.y;
    if (w.ctrl[0] != 0 || w.state[j].done) return;                          // uniform over the workgroup
    const int src = jobs[2 * j], tgt = jobs[2 * j + 1];
    const int64_t lo = offsets[src], hi = offsets[src + 1];
    const int64_t per = (hi - lo + w.slices - 1) / w.slices;
    const int64_t a = lo + slice * per, b = a + per < hi ? a + per : hi;
    IcpGrid g;
    g.keys = w.keys; g.start = w.start; g.list = w.list; g.points = points; g.mask = w.slots - 1; g.n = n; g.n_list = n; g.h = h;
    double T[12];
    for (int k = 0; k < 12; ++k) T[k] = w.state[j].T[k];
    double acc[ICP_SUMS];
    for (int k = 0; k < ICP_SUMS; ++k) acc[k] = 0.0;
    for (int64_t i = a + threadIdx.x; i < b; i += ICP_BLOCK) {
        double q[3], d2;
        icp_apply(T, points + 3 * i, q);
        const int64_t m = icp_nearest(g, tgt, q, thr2, &d2);
        if (m < 0) continue;
        const double t[3] = {(double)points[3 * m], (double)points[3 * m + 1], (double)points[3 * m + 2]};
        acc[0] += 1.0;
        for (int c = 0; c < 3; ++c) {
            acc[1 + c] += q[c];
            acc[4 + c] += t[c];
            for (int d = 0; d < 3; ++d) acc[7 + 3 * c + d] += t[c] * q[d];
        }
        acc[16] += d2;
    }
    for (int k = 0; k < ICP_SUMS; ++k) red[k][threadIdx.x] = acc[k];
    __syncthreads();
    for (int s = ICP_BLOCK / 2; s > 0; s >>= 1) {                           // fixed tree: the same order every run
        if ((int)threadIdx.x < s)
            for (int k = 0; k < ICP_SUMS; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < ICP_SUMS) w.partial[((int64_t)j * w.slices + slice) * ICP_SUMS + threadIdx.x] = red[threadIdx.x][0];
}

// A = U diag(sigma) V^T of a 3x3 by one-sided Jacobi rotations of the columns; the rotation U S V^T with S = diag(1, 1, +-1), the -1 on the
// smallest singular value when det(U) det(V) < 0 (Umeyama's reflection fix).  Columns of U whose singular value vanishes against the largest
// (fewer than three non-collinear correspondences) are completed to a right-handed orthonormal basis: always a finite proper rotation, and the
// same one every run; A = 0 gives the identity.  `noise` is the rounding noise of the covariance (it is formed from uncentred float64 sums:
// sum t q^T / k - mean t mean q^T): a singular value at or below it counts as zero, so that a covariance that is zero in exact arithmetic -- every
// source point matched to ONE target point -- gives the identity and not a rotation read out of rounding errors.  Returns true when a column
// had to be completed.
__device__ bool icp_rotation(const double cov[9], double noise, double R[9])
{
#pragma clang fp contract(off)
    double A[3][3], V[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) { A[r][c] = cov[3 * r + c]; V[r][c] = r == c ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int k = 0; k < 3; ++k) { alpha += A[k][p] * A[k][p]; beta += A[k][q] * A[k][q]; gamma += A[k][p] * A[k][q]; }
                if (gamma == 0.0 || fabs(gamma) <= 1e-17 * sqrt(alpha * beta)) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int k = 0; k < 3; ++k) {
                    const double ap = A[k][p], aq = A[k][q], vp = V[k][p], vq = V[k][q];
                    A[k][p] = c * ap - s * aq; A[k][q] = s * ap + c * aq;
                    V[k][p] = c * vp - s * vq; V[k][q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    double sig[3];
    for (int c = 0; c < 3; ++c) sig[c] = sqrt(A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c]);
    int i0 = 0, i1 = 1, i2 = 2, tmp;                                          // sigma descending, ties by column index
    if (sig[i1] > sig[i0]) { tmp = i0; i0 = i1; i1 = tmp; }
    if (sig[i2] > sig[i1]) { tmp = i1; i1 = i2; i2 = tmp; }
    if (sig[i1] > sig[i0]) { tmp = i0; i0 = i1; i1 = tmp; }
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    if (!(sig[i0] > noise) || !icp_finite(sig[i0])) return true;
    double tol = 64.0 * 2.220446049250313e-16 * sig[i0];
    if (tol < noise) tol = noise;
    double U[3][3];
    bool completed = false;
    for (int k = 0; k < 3; ++k) U[k][i0] = A[k][i0] / sig[i0];
    if (sig[i1] > tol) {
        for (int k = 0; k < 3; ++k) U[k][i1] = A[k][i1] / sig[i1];
    } else {                                                                  // any unit vector orthogonal to u0: u0 x e_m, m the axis u0 leans on least
        completed = true;
        int m = 0;
        if (fabs(U[1][i0]) < fabs(U[m][i0])) m = 1;
        if (fabs(U[2][i0]) < fabs(U[m][i0])) m = 2;
        double e[3] = {0.0, 0.0, 0.0};
        e[m] = 1.0;
        double v[3] = {U[1][i0] * e[2] - U[2][i0] * e[1], U[2][i0] * e[0] - U[0][i0] * e[2], U[0][i0] * e[1] - U[1][i0] * e[0]};
        const double nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        for (int k = 0; k < 3; ++k) U[k][i1] = v[k] / nv;
    }
    if (sig[i2] > tol) {
        for (int k = 0; k < 3; ++k) U[k][i2] = A[k][i2] / sig[i2];
    } else {
        completed = true;
        U[0][i2] = U[1][i0] * U[2][i1] - U[2][i0] * U[1][i1];
        U[1][i2] = U[2][i0] * U[0][i1] - U[0][i0] * U[2][i1];
        U[2][i2] = U[0][i0] * U[1][i1] - U[1][i0] * U[0][i1];
    }
    auto det3 = [](const double M[3][3]) {
        return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
               M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
    };
    double S[3] = {1.0, 1.0, 1.0};
    if (det3(U) * det3(V) < 0.0) S[i2] = -1.0;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double v = 0.0;
            for (int k = 0; k < 3; ++k) v += U[r][k] * S[k] * V[c][k];
            R[3 * r + c] = v;
        }
    for (int k = 0; k < 9; ++k)
        if (!icp_finite(R[k])) {
            for (int m = 0; m < 9; ++m) R[m] = (m % 4 == 0) ? 1.0 : 0.0;
            return true;
        }
    return completed;
}

__global__ __launch_bounds__(64) void icp_update(const int32_t *__restrict__ offsets, const int32_t *__restrict__ jobs, int round, int max_iter,
                                                 IcpWs w, double *__restrict__ out_T, double *__restrict__ out_fit, double *__restrict__ out_rmse,
                                                 int32_t *__restrict__ out_iters, int32_t *__restrict__ out_status)
{
#pragma clang fp contract(off)
    __shared__ double sums[ICP_SUMS];
    const int j = blockIdx.x;
    IcpState &st = w.state[j];
    if (w.ctrl[0] != 0) {                                                   // a table that cannot be trusted: identity, and the status says so
        if (threadIdx.x == 0 && round == 0) {
            for (int k = 0; k < 16; ++k) out_T[16 * (int64_t)j + k] = (k % 5 == 0) ? 1.0 : 0.0;
            out_fit[j] = out_rmse[j] = 0.0;
            out_iters[j] = 0;
            out_status[j] = PCACC_ICP_BAD_TABLE;
        }
        return;
    }
    if (st.done) return;
    if (threadIdx.x < ICP_SUMS) {
        double v = 0.0;
        for (int s = 0; s < w.slices; ++s) v += w.partial[((int64_t)j * w.slices + s) * ICP_SUMS + threadIdx.x];     // slice order
        sums[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int src = jobs[2 * j], tgt = jobs[2 * j + 1];
    const int64_t n_src = (int64_t)offsets[src + 1] - offsets[src], n_tgt = (int64_t)offsets[tgt + 1] - offsets[tgt];
    const double nc = sums[0];
    const double fit = n_src > 0 ? nc / (double)n_src : 0.0;
    const double rmse = nc > 0.0 ? sqrt(sums[16] / nc) : 0.0;
    int status = st.status | (n_src == 0 ? PCACC_ICP_EMPTY_SOURCE : 0) | (n_tgt == 0 ? PCACC_ICP_EMPTY_TARGET : 0);
    const bool converged = round > 0 && fabs(fit - st.fit) < 1e-6 && fabs(rmse - st.rmse) < 1e-6;
    if (converged || round >= max_iter) {
        if (!(nc > 0.0)) status |= PCACC_ICP_NO_CORRESPONDENCE;
        for (int k = 0; k < 16; ++k) out_T[16 * (int64_t)j + k] = st.T[k];
        out_fit[j] = fit;
        out_rmse[j] = rmse;
        out_iters[j] = round;
        out_status[j] = status;
        st.status = status;
        st.done = 1;
        return;
    }
    if (nc > 0.0) {                                                         // no correspondences: the update is the identity
        double ms[3], mt[3], cov[9], R[9], t[3];
        for (int c = 0; c < 3; ++c) { ms[c] = sums[1 + c] / nc; mt[c] = sums[4 + c] / nc; }
        for (int c = 0; c < 3; ++c)
            for (int d = 0; d < 3; ++d) cov[3 * c + d] = sums[7 + 3 * c + d] / nc - mt[c] * ms[d];
        // 1e-10 of the mean of t . q: far above the rounding of the sums (2^-53 times at most the number of terms), far below the covariance of
        // any cloud that has an extent (a singular value of 1e-10 of the squared distance from the origin is a thickness of micrometres)
        const double noise = 1e-10 * (fabs(sums[7]) + fabs(sums[11]) + fabs(sums[15])) / nc;
        if (icp_rotation(cov, noise, R)) status |= PCACC_ICP_RANK_DEFICIENT;
        for (int c = 0; c < 3; ++c) t[c] = mt[c] - (R[3 * c] * ms[0] + R[3 * c + 1] * ms[1] + R[3 * c + 2] * ms[2]);
        double N[12];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c)
                N[4 * r + c] = R[3 * r] * st.T[c] + R[3 * r + 1] * st.T[4 + c] + R[3 * r + 2] * st.T[8 + c] + (c == 3 ? t[r] : 0.0);
        for (int k = 0; k < 12; ++k) st.T[k] = N[k];
    }
    st.fit = fit;
    st.rmse = rmse;
    st.iters = round + 1;
    st.status = status;
}

extern "C" int pcacc_icp_point_to_point(const float *points, int64_t n, const int32_t *seg_offsets, int32_t n_seg, const int32_t *jobs,
                                        int32_t n_jobs, const double *init, double threshold, int32_t max_iter, double *out_T,
                                        double *out_fitness, double *out_rmse, int32_t *out_iters, int32_t *out_status, void *ws, size_t ws_bytes,
                                        void *stream)
{
    if (!icp_sizes_ok(n, n_seg, n_jobs, max_iter) || !seg_offsets || !ws) return PCACC_E_ARG;
    if (!(threshold > 0.0) || !(threshold < 1e300)) return PCACC_E_ARG;
    if (n > 0 && !points) return PCACC_E_ARG;
    if (n_jobs == 0) return 0;
    if (!jobs || !out_T || !out_fitness || !out_rmse || !out_iters || !out_status) return PCACC_E_ARG;
    IcpWs w;
    const size_t need = icp_carve(&w, (char *)ws, n, n_seg, n_jobs);
    if (ws_bytes < need) return PCACC_E_WORKSPACE;
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(ws, 0, w.zero_bytes, st) != hipSuccess) return PCACC_E_LAUNCH;
    const int setup_items = n_jobs > n_seg + 1 ? n_jobs : n_seg + 1;
    hipLaunchKernelGGL(icp_setup, dim3((setup_items + ICP_BLOCK - 1) / ICP_BLOCK), dim3(ICP_BLOCK), 0, st, seg_offsets, n_seg, jobs, n_jobs, n, init, w);
    if (n > 0) hipLaunchKernelGGL(icp_insert, dim3(pcacc_grid(n, ICP_BLOCK)), dim3(ICP_BLOCK), 0, st, points, n, seg_offsets, n_seg, threshold, w);
    const int chunks = pcacc_chunks(w.slots);
    hipLaunchKernelGGL(chunk_sums_i32, dim3(chunks), dim3(256), 0, st, w.cnt, (int64_t)w.slots, w.sums);
    hipLaunchKernelGGL(scan_chunk_sums, dim3(1), dim3(1024), 0, st, w.sums, chunks, (int *)nullptr, -1);
    hipLaunchKernelGGL(chunk_scan_i32, dim3(chunks), dim3(256), 0, st, w.cnt, (int64_t)w.slots, w.sums, w.start, 1, w.cnt);
    if (n > 0) hipLaunchKernelGGL(icp_fill, dim3(pcacc_grid(n, ICP_BLOCK)), dim3(ICP_BLOCK), 0, st, n, w);
    PCACC_CHECK_LAUNCH();
    const double thr2 = threshold * threshold;
    for (int round = 0; round <= max_iter; ++round) {
        hipLaunchKernelGGL(icp_corr, dim3(n_jobs, w.slices), dim3(ICP_BLOCK), 0, st, points, n, seg_offsets, jobs, threshold, thr2, w);
        hipLaunchKernelGGL(icp_update, dim3(n_jobs), dim3(64), 0, st, seg_offsets, jobs, round, max_iter, w, out_T, out_fitness, out_rmse,
                           out_iters, out_status);
    }
    PCACC_CHECK_LAUNCH();
    return 0;
}
