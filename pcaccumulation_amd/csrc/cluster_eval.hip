// C2. Instance-segmentation evaluation of the test loop -- toolbox/cluster_eval.py:71-152 (ClusterEvaluation.forward) for every sample of a
// batch at once (libs/loss.py:261-270).  The reference walks all (estimated, ground-truth) instance pairs and builds two masks of length N per
// pair; everything it reads off those masks is a function of four integer tables:
//   per (sample, estimated id) and per (sample, ground-truth id): the number of points and the number of moving points,
//   per non-empty (estimated, ground-truth) pair of a sample:     the number of common points.
// One pass over the points fills them, a pass over the pairs turns them into the best IoU of every instance.
//
//   eval_points   instance rows are found through two open-addressing hash tables keyed (sample, id); a new key takes the next dense row of
//                 the output table.  A wave first groups its 64 points by (sample, est, gt) with ballots (no memory traffic), then one lane
//                 per group adds the group's counts: row count | moving count as ONE 64-bit integer add, the pair's count into a third table
//                 keyed (est row, gt row).  Points that are background on both sides -- most of a scene -- touch nothing.
//   eval_classes  class of every row (1 iff 2 * moving > count: Python's round() of the fp32 mean, ties to even), ground-truth instances per
//                 (sample, class), the 2^24 points-per-sample limit below which that integer rule IS the reference's fp32 mean.
//   eval_pairs    IoU = fp32(inter) / fp32(|est| + |gt| - inter), one IEEE division, for the pairs of equal class; integer atomicMax on its
//                 bit pattern (positive floats order like their bits) into both rows.
//   eval_finish   -1.0 for estimated instances whose class has no ground-truth instance in the sample; the header.
// Only integer atomics: two runs give the same tables up to the order of the rows, which the host sorts by (sample, id) anyway.
//
// Visibility inside eval_points.  The per-XCD L2s are not coherent and a slot's key is 12 bytes, so a slot cannot be published by one CAS.
// Every word of a slot is instead WRITE-ONCE (0 = not written yet: ids are non-zero, sample and row are stored + 1), written with a device-scope
// atomic exchange and read with a device-scope atomic load: a reader that sees a non-zero word sees its final value, one that sees 0 asks
// again.  No fence, no ordering between the words is needed.  A lane never waits inside an iteration of the probe loop (the slot's owner
// writes all three words in the iteration that won the slot), so lanes of one wave cannot wait for each other.
#include "common.h"

#define CE_BLOCK 256
#define CE_HEADER_WORDS 16
#define CE_ST_INST 1       // more instances than inst_capacity
#define CE_ST_PAIR 2       // more non-empty pairs than pair_capacity
#define CE_ST_SAMPLE 4     // a sample with more than 2^24 points
#define CE_ST_BATCH 8      // a batch index outside [0, n_batches)

struct CeRow {             // 32 bytes; pcaccumulation_amd/cluster_eval.py: ROW_DTYPE
    int64_t id;
    uint32_t count, ones;  // one 64-bit word for the point pass
    int32_t sample, cls;
    float best;
    int32_t pad;
};

struct CeTable {           // open addressing, linear probing, `mask` + 1 slots
    int32_t *sample1;      // sample + 1; the word a slot is won on
    unsigned long long *id;
    int32_t *row1;         // row + 1
    uint32_t mask;
};

struct CeWs {
    int32_t *ctrl;         // [0] estimated rows, [1] ground-truth rows, [2] pairs, [3] status
    uint32_t *sample_cnt;  // [n_batches]
    uint32_t *gt_classes;  // [n_batches][2]
    CeTable est, gt;
    unsigned long long *pair_key;   // ((est row << 32) | gt row) + 1
    uint32_t *pair_cnt;
    uint32_t pair_mask;
};

static uint32_t ce_pow2(int64_t v)
{
    uint32_t p = 64;
    while ((int64_t)p < v) p <<= 1;
    return p;
}

static size_t ce_carve(CeWs *w, char *base, int32_t n_batches, int32_t inst_capacity, int32_t pair_capacity)
{
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += pcacc_align(bytes); return p; };
    const uint32_t slots = ce_pow2(2ll * inst_capacity), pslots = ce_pow2(2ll * pair_capacity);
    w->ctrl = (int32_t *)take(CE_HEADER_WORDS * 4);
    w->sample_cnt = (uint32_t *)take((size_t)n_batches * 4);
    w->gt_classes = (uint32_t *)take((size_t)n_batches * 8);
    for (CeTable *t : {&w->est, &w->gt}) {
        t->sample1 = (int32_t *)take((size_t)slots * 4);
        t->id = (unsigned long long *)take((size_t)slots * 8);
        t->row1 = (int32_t *)take((size_t)slots * 4);
        t->mask = slots - 1;
    }
    w->pair_key = (unsigned long long *)take((size_t)pslots * 8);
    w->pair_cnt = (uint32_t *)take((size_t)pslots * 4);
    w->pair_mask = pslots - 1;
    return off;
}

static bool ce_sizes_ok(int64_t n, int32_t n_batches, int32_t inst_capacity, int32_t pair_capacity)
{
    return n >= 0 && n < (1ll << 31) - 1 && n_batches >= 1 && n_batches <= (1 << 20) && inst_capacity >= 1 && inst_capacity <= (1 << 28) &&
           pair_capacity >= 1 && pair_capacity <= (1 << 28);
}

extern "C" int pcacc_cluster_eval_workspace_bytes(int64_t n, int32_t n_batches, int32_t inst_capacity, int32_t pair_capacity, size_t *bytes)
{
    if (!bytes || !ce_sizes_ok(n, n_batches, inst_capacity, pair_capacity)) return PCACC_E_ARG;
    CeWs w;
    *bytes = ce_carve(&w, nullptr, n_batches, inst_capacity, pair_capacity);
    return 0;
}

__device__ __forceinline__ uint64_t ce_mix(uint64_t x)      // the 64-bit finaliser of MurmurHash3
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    return x ^ (x >> 33);
}

template <class T>
__device__ __forceinline__ T ce_load(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Row of (sample, id) in `rows`, created on first sight; -1 when the table was sized too small (status says so, the caller's result is void).
__device__ int ce_row(const CeTable &t, int sample, int64_t id, CeRow *rows, int capacity, int32_t *n_rows, int32_t *status)
{
    uint32_t h = (uint32_t)ce_mix((uint64_t)id ^ ((uint64_t)(sample + 1) * 0x9e3779b97f4a7c15ull)) & t.mask;
    uint32_t probes = 0;
    while (probes <= t.mask) {
        int32_t s = ce_load(&t.sample1[h]);
        if (s == 0) s = atomicCAS(&t.sample1[h], 0, sample + 1);
        if (s == 0) {                                                      // this lane won the slot: all of it is written before the lane moves on
            const int r = atomicAdd(n_rows, 1);
            atomicExch(&t.id[h], (unsigned long long)id);
            atomicExch(&t.row1[h], r + 1);
            if (r >= capacity) { atomicOr(status, CE_ST_INST); return -1; }
            rows[r].id = id;                                               // read by the kernels behind this one only
            rows[r].sample = sample;
            return r;
        }
        if (s == sample + 1) {
            const unsigned long long k = ce_load(&t.id[h]);
            if (k == 0) continue;                                          // its owner is between the two writes: ask again
            if (k == (unsigned long long)id) {
                const int r1 = ce_load(&t.row1[h]);
                if (r1 == 0) continue;
                return r1 - 1 < capacity ? r1 - 1 : -1;
            }
        }
        h = (h + 1) & t.mask;
        if ((++probes & 63) == 0 && ce_load(status) != 0) return -1;       // an overfull table: every probe sequence is long, and the result void
    }
    atomicOr(status, CE_ST_INST);
    return -1;
}

__device__ void ce_pair_add(const CeWs &w, int er, int gr, uint32_t cnt, int pair_capacity)
{
    const unsigned long long key = (((unsigned long long)er << 32) | (uint32_t)gr) + 1;
    uint32_t h = (uint32_t)ce_mix(key) & w.pair_mask;
    for (uint32_t probes = 0; probes <= w.pair_mask; ++probes, h = (h + 1) & w.pair_mask) {
        unsigned long long k = ce_load(&w.pair_key[h]);
        if (k == 0) {
            k = atomicCAS(&w.pair_key[h], 0ull, key);
            if (k == 0) {
                if (atomicAdd(&w.ctrl[2], 1) >= pair_capacity) atomicOr(&w.ctrl[3], CE_ST_PAIR);
                k = key;
            }
        }
        if (k == key) { atomicAdd(&w.pair_cnt[h], cnt); return; }
        if ((probes & 63) == 63 && ce_load(&w.ctrl[3]) != 0) return;
    }
    atomicOr(&w.ctrl[3], CE_ST_PAIR);
}

template <int MOS>
__device__ __forceinline__ bool ce_moving(const void *mos, int64_t i)
{
    if (MOS == PCACC_MOS_I64) return reinterpret_cast<const int64_t *>(mos)[i] != 0;
    if (MOS == PCACC_MOS_F32) return reinterpret_cast<const float *>(mos)[i] != 0.f;
    return reinterpret_cast<const uint8_t *>(mos)[i] != 0;
}

template <int MOS>
__global__ __launch_bounds__(CE_BLOCK) void eval_points(const int64_t *__restrict__ inst_est, const int64_t *__restrict__ inst_gt,
                                                        const void *__restrict__ mos, const int32_t *__restrict__ batch, int64_t n,
                                                        int n_batches, CeWs w, CeRow *est_rows, CeRow *gt_rows, int inst_capacity,
                                                        int pair_capacity)
{
    const int lane = lane_id();
    int run_sample = -1;                 // wave-uniform: points of one sample seen by this wave and not yet added to sample_cnt
    uint32_t run_cnt = 0;
    for (int64_t base = (int64_t)blockIdx.x * CE_BLOCK; base < n; base += (int64_t)gridDim.x * CE_BLOCK) {
        const int64_t i = base + threadIdx.x;
        bool valid = i < n;
        int b = valid ? batch[i] : 0;
        if (valid && (b < 0 || b >= n_batches)) {
            atomicOr(&w.ctrl[3], CE_ST_BATCH);
            valid = false;
        }
        const int64_t e = valid ? inst_est[i] : 0, g = valid ? inst_gt[i] : 0;
        const bool mv = valid && (e != 0 || g != 0) && ce_moving<MOS>(mos, i);

        // points per sample: a wave nearly always sits inside one sample (collate_fn concatenates the samples)
        const uint64_t vmask = __ballot(valid);
        if (vmask) {
            const int b0 = __shfl(b, __builtin_ctzll(vmask), 64);
            if (__ballot(valid && b != b0) == 0) {
                if (b0 != run_sample) {
                    if (run_cnt && lane == 0) atomicAdd(&w.sample_cnt[run_sample], run_cnt);
                    run_sample = b0;
                    run_cnt = 0;
                }
                run_cnt += __popcll(vmask);
            } else if (valid) {
                atomicAdd(&w.sample_cnt[b], 1u);
            }
        }

        // groups of equal (sample, est, gt) inside the wave: the lowest lane of a group carries its two counts
        const bool need = valid && (e != 0 || g != 0);
        uint64_t rem = __ballot(need);
        bool leader = false;
        uint32_t cnt = 0, ones = 0;
        while (rem) {
            const int l = __builtin_ctzll(rem);
            const int64_t le = __shfl(e, l, 64), lg = __shfl(g, l, 64);
            const int lb = __shfl(b, l, 64);
            const bool same = need && e == le && g == lg && b == lb;
            const uint64_t m = __ballot(same), mo = __ballot(same && mv);
            if (lane == l) {
                leader = true;
                cnt = __popcll(m);
                ones = __popcll(mo);
            }
            rem &= ~m;
        }
        if (leader) {
            const unsigned long long add = (unsigned long long)cnt | ((unsigned long long)ones << 32);
            int er = -1, gr = -1;
            if (e != 0) {
                er = ce_row(w.est, b, e, est_rows, inst_capacity, &w.ctrl[0], &w.ctrl[3]);
                if (er >= 0) atomicAdd(reinterpret_cast<unsigned long long *>(&est_rows[er].count), add);
            }
            if (g != 0) {
                gr = ce_row(w.gt, b, g, gt_rows, inst_capacity, &w.ctrl[1], &w.ctrl[3]);
                if (gr >= 0) atomicAdd(reinterpret_cast<unsigned long long *>(&gt_rows[gr].count), add);
            }
            if (er >= 0 && gr >= 0) ce_pair_add(w, er, gr, cnt, pair_capacity);
        }
    }
    if (run_cnt && lane == 0) atomicAdd(&w.sample_cnt[run_sample], run_cnt);
}

__device__ __forceinline__ int ce_rows_used(const int32_t *ctrl, int which, int capacity) { return min(max(ctrl[which], 0), capacity); }

__global__ __launch_bounds__(CE_BLOCK) void eval_classes(CeWs w, CeRow *est_rows, CeRow *gt_rows, int inst_capacity, int n_batches)
{
    const int n_est = ce_rows_used(w.ctrl, 0, inst_capacity), n_gt = ce_rows_used(w.ctrl, 1, inst_capacity);
    const int stride = gridDim.x * CE_BLOCK, t0 = blockIdx.x * CE_BLOCK + threadIdx.x;
    for (int r = t0; r < n_est; r += stride) est_rows[r].cls = 2ull * est_rows[r].ones > est_rows[r].count ? 1 : 0;
    for (int r = t0; r < n_gt; r += stride) {
        const int cls = 2ull * gt_rows[r].ones > gt_rows[r].count ? 1 : 0;
        gt_rows[r].cls = cls;
        atomicAdd(&w.gt_classes[2 * gt_rows[r].sample + cls], 1u);
    }
    for (int b = t0; b < n_batches; b += stride)
        if (w.sample_cnt[b] > (1u << 24)) atomicOr(&w.ctrl[3], CE_ST_SAMPLE);
}

__global__ __launch_bounds__(CE_BLOCK) void eval_pairs(CeWs w, CeRow *est_rows, CeRow *gt_rows, int inst_capacity)
{
#pragma clang fp contract(off)
    const int n_est = ce_rows_used(w.ctrl, 0, inst_capacity), n_gt = ce_rows_used(w.ctrl, 1, inst_capacity);
    for (uint32_t s = blockIdx.x * CE_BLOCK + threadIdx.x; s <= w.pair_mask; s += gridDim.x * CE_BLOCK) {
        const unsigned long long key = w.pair_key[s];
        if (key == 0) continue;
        const int er = (int)((key - 1) >> 32), gr = (int)((key - 1) & 0xffffffffull);
        if (er >= n_est || gr >= n_gt || est_rows[er].cls != gt_rows[gr].cls) continue;
        const uint32_t inter = w.pair_cnt[s];
        const uint32_t uni = est_rows[er].count + gt_rows[gr].count - inter;
        const float iou = (float)inter / (float)uni;                       // both conversions and the division round to nearest: torch's int64 / int64
        atomicMax(reinterpret_cast<int *>(&est_rows[er].best), __float_as_int(iou));
        atomicMax(reinterpret_cast<int *>(&gt_rows[gr].best), __float_as_int(iou));
    }
}

__global__ __launch_bounds__(CE_BLOCK) void eval_finish(CeWs w, CeRow *est_rows, int inst_capacity, int32_t *header)
{
    const int n_est = ce_rows_used(w.ctrl, 0, inst_capacity);
    for (int r = blockIdx.x * CE_BLOCK + threadIdx.x; r < n_est; r += gridDim.x * CE_BLOCK)
        if (w.gt_classes[2 * est_rows[r].sample + est_rows[r].cls] == 0) est_rows[r].best = -1.f;      // cluster_eval.py:135: no candidate at all
    if (blockIdx.x == 0 && threadIdx.x < 4) header[threadIdx.x] = w.ctrl[(threadIdx.x + 3) & 3];      // status, estimated rows, ground-truth rows, pairs
}

extern "C" int pcacc_cluster_eval(const int64_t *inst_est, const int64_t *inst_gt, const void *mos, int32_t mos_dtype, const int32_t *batch,
                                  int64_t n, int32_t n_batches, int32_t inst_capacity, int32_t pair_capacity, void *out, size_t out_bytes,
                                  void *ws, size_t ws_bytes, void *stream)
{
    if (!ce_sizes_ok(n, n_batches, inst_capacity, pair_capacity) || !out || !ws) return PCACC_E_ARG;
    if (mos_dtype != PCACC_MOS_I64 && mos_dtype != PCACC_MOS_F32 && mos_dtype != PCACC_MOS_U8) return PCACC_E_ARG;
    if (n > 0 && (!inst_est || !inst_gt || !mos || !batch)) return PCACC_E_ARG;
    if (n > (int64_t)n_batches << 24) return PCACC_E_ARG;                  // some sample has more than 2^24 points whatever the batch column says
    const size_t need_out = CE_HEADER_WORDS * 4 + 2 * (size_t)inst_capacity * sizeof(CeRow);
    if (out_bytes < need_out) return PCACC_E_ARG;
    CeWs w;
    const size_t need_ws = ce_carve(&w, (char *)ws, n_batches, inst_capacity, pair_capacity);
    if (ws_bytes < need_ws) return PCACC_E_WORKSPACE;
    hipStream_t st = pcacc_stream(stream);
    if (hipMemsetAsync(ws, 0, need_ws, st) != hipSuccess || hipMemsetAsync(out, 0, need_out, st) != hipSuccess) return PCACC_E_LAUNCH;
    int32_t *header = (int32_t *)out;
    CeRow *est_rows = (CeRow *)((char *)out + CE_HEADER_WORDS * 4), *gt_rows = est_rows + inst_capacity;
    if (n > 0) {
        const int grid = pcacc_grid(n, CE_BLOCK);
        if (mos_dtype == PCACC_MOS_I64)
            hipLaunchKernelGGL(eval_points<PCACC_MOS_I64>, dim3(grid), dim3(CE_BLOCK), 0, st, inst_est, inst_gt, mos, batch, n, n_batches, w,
                               est_rows, gt_rows, inst_capacity, pair_capacity);
        else if (mos_dtype == PCACC_MOS_F32)
            hipLaunchKernelGGL(eval_points<PCACC_MOS_F32>, dim3(grid), dim3(CE_BLOCK), 0, st, inst_est, inst_gt, mos, batch, n, n_batches, w,
                               est_rows, gt_rows, inst_capacity, pair_capacity);
        else
            hipLaunchKernelGGL(eval_points<PCACC_MOS_U8>, dim3(grid), dim3(CE_BLOCK), 0, st, inst_est, inst_gt, mos, batch, n, n_batches, w,
                               est_rows, gt_rows, inst_capacity, pair_capacity);
        const int rows_grid = pcacc_grid(inst_capacity > n_batches ? inst_capacity : n_batches, CE_BLOCK, PCACC_CUS * 4);
        hipLaunchKernelGGL(eval_classes, dim3(rows_grid), dim3(CE_BLOCK), 0, st, w, est_rows, gt_rows, inst_capacity, n_batches);
        hipLaunchKernelGGL(eval_pairs, dim3(pcacc_grid((int64_t)w.pair_mask + 1, CE_BLOCK, PCACC_CUS * 4)), dim3(CE_BLOCK), 0, st, w, est_rows,
                           gt_rows, inst_capacity);
        hipLaunchKernelGGL(eval_finish, dim3(rows_grid), dim3(CE_BLOCK), 0, st, w, est_rows, inst_capacity, header);
    }
    PCACC_CHECK_LAUNCH();
    return 0;
}
