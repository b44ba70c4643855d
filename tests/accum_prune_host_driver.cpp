// Host build of pcaccumulation_amd/csrc/accum_prune.h (tests/test_accumulate_prune.py): the reason of a row, the neighbour count of a survivor and the
// move of a surviving row -- the functions the kernels of accum_prune.hip call -- run on the CPU with every table index assert-checked
// (-DPCACC_HOST_CHECK), before anything runs on a GPU.  The steps between them (flags, exclusive scan, dst / rows, second scan) are the kernels' steps.
// The input tables stand at their capacity with poison behind row m that no result may depend on; the output tables are poison everywhere before
// the compaction: every destination below `kept` is written exactly once, keys ascend, and the poison behind row `kept` is untouched.
//   in : i64 m, in_capacity, out_capacity, has_pierced, min_count, use_fraction, use_stamp, before_stamp, use_box, lo[3], hi[3], min_pierced, use_ratio,
//        min_neighbors, radius; f64 max_moving_fraction, ratio; i64 keys[m]; i64 acc[5][m]; i32 stamps[2][m]; i32 pierced[m] (has_pierced)
//   out: i64 counters[6]; i64 keys[kept]; i64 acc[5][kept]; i32 stamps[2][kept]; i32 pierced[kept] (has_pierced); i32 k[m] (stage B's count of a
//        stage-A survivor, else -1); u8 reason[m]
#include <cassert>
#include <cstdio>
#include <vector>

#include "accum_prune.h"

typedef unsigned long long u64;

#define POISON_KEY 0x5a5a5a5a5a5a5a5aull
#define POISON_ACC 0x5b5b5b5b5b5b5b5bll
#define POISON_I32 0x5c5c5c5c

template <class T> static std::vector<T> rd(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n) assert(fread(v.data(), sizeof(T), n, f) == n);
    return v;
}

template <class T> static void wr(FILE *f, const std::vector<T> &v)
{
    if (!v.empty()) assert(fwrite(v.data(), sizeof(T), v.size(), f) == v.size());
}

// kpos[0..m] = exclusive scan of flag, kpos[m] = total
static std::vector<int> scan(const std::vector<int> &flag)
{
    std::vector<int> kpos(flag.size() + 1, 0);
    for (size_t i = 0; i < flag.size(); ++i) kpos[i + 1] = kpos[i] + flag[i];
    return kpos;
}

int main(int argc, char **argv)
{
    assert(argc == 3);
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    assert(f && o);
    const std::vector<int64_t> h = rd<int64_t>(f, 19);
    const std::vector<double> g = rd<double>(f, 2);
    const int64_t m = h[0], cap = h[1], ocap = h[2];
    const bool has_pierced = h[3] != 0;
    AccrParams P;
    P.min_count = h[4]; P.use_fraction = h[5] != 0; P.use_stamp = h[6] != 0; P.before_stamp = (int32_t)h[7]; P.use_box = h[8] != 0;
    P.lo_x = (int32_t)h[9]; P.lo_y = (int32_t)h[10]; P.lo_z = (int32_t)h[11]; P.hi_x = (int32_t)h[12]; P.hi_y = (int32_t)h[13]; P.hi_z = (int32_t)h[14];
    P.min_pierced = (int32_t)h[15]; P.use_ratio = h[16] != 0; P.max_moving_fraction = g[0]; P.ratio = g[1];
    const int min_neighbors = (int)h[17], radius = (int)h[18];
    assert(m >= 0 && cap >= m && cap >= 1 && ocap >= m && ocap >= 1 && min_neighbors >= 0 && min_neighbors <= ACCR_MAX_NEIGHBORS);
    assert(min_neighbors == 0 || (radius >= 1 && radius <= ACCN_MAX_RADIUS));
    // rows past m: a key that would mislead any search that read it, a record that passes every filter
    std::vector<u64> keys(cap, 0);
    std::vector<int64_t> acc((size_t)ACC_FIELDS * cap, 1000);
    std::vector<int32_t> stamps(2 * cap, 0x7fffffff), pierced(has_pierced ? cap : 0, 0);
    {
        const std::vector<int64_t> k = rd<int64_t>(f, m), a = rd<int64_t>(f, (size_t)ACC_FIELDS * m);
        const std::vector<int32_t> s = rd<int32_t>(f, 2 * m), p = rd<int32_t>(f, has_pierced ? m : 0);
        for (int64_t i = 0; i < m; ++i) {
            keys[i] = (u64)k[i];
            assert(i == 0 || keys[i - 1] < keys[i]);
            for (int c = 0; c < ACC_FIELDS; ++c) acc[(size_t)c * cap + i] = a[(size_t)c * m + i];
            stamps[i] = s[i];
            stamps[cap + i] = s[m + i];
            if (has_pierced) pierced[i] = p[i];
        }
    }
    const int32_t *pin = has_pierced ? pierced.data() : nullptr;

    // stage A
    std::vector<int> flag(m);
    std::vector<uint8_t> reason(m);
    for (int64_t i = 0; i < m; ++i) {
        const int r = accr_row_reason(keys.data(), acc.data(), stamps.data(), pin, cap, m, i, P);
        assert(r >= ACCR_KEPT && r <= ACCR_PIERCED);
        flag[i] = r == ACCR_KEPT;
        reason[i] = (uint8_t)r;
    }
    std::vector<int> kpos = scan(flag);
    // stage B
    std::vector<int32_t> kout(m, -1);
    if (min_neighbors > 0) {
        const int64_t alive = kpos[m];
        std::vector<int> dst(m, -1), rows(alive, -1);
        for (int64_t i = 0; i < m; ++i) {
            const int64_t d = flag[i] ? accum_merge_dst(kpos[i], 0, alive) : -1;
            dst[i] = (int)d;
            if (d >= 0) { PCACC_BOUND(d, alive); assert(rows[d] == -1); rows[d] = (int)i; }
        }
        for (int64_t j = 0; j < alive; ++j) {
            const int64_t i = rows[j];
            assert(i >= 0 && i < m && dst[i] == j);
            const int k = accr_neighbors(keys.data(), m, dst.data(), i, radius);
            assert(k >= 1 && k <= (2 * radius + 1) * (2 * radius + 1) * (2 * radius + 1));
            kout[i] = k;
            if (k < min_neighbors) { flag[i] = 0; reason[i] = ACCR_ISOLATED; }
        }
        kpos = scan(flag);
    }
    // compaction
    const int64_t kept = kpos[m];
    std::vector<u64> okeys(ocap, POISON_KEY);
    std::vector<int64_t> oacc((size_t)ACC_FIELDS * ocap, POISON_ACC);
    std::vector<int32_t> ostamps(2 * ocap, POISON_I32), opierced(has_pierced ? ocap : 0, POISON_I32);
    std::vector<int> written(ocap, 0);
    std::vector<int64_t> counters(ACCR_REASONS, 0);
    for (int64_t i = 0; i < m; ++i) {
        counters[reason[i]] += 1;
        if (!flag[i]) continue;
        const int64_t d = accum_merge_dst(kpos[i], 0, kept);
        assert(d >= 0 && d < kept);
        assert(accr_move_row(keys.data(), acc.data(), stamps.data(), pin, cap, m, i, okeys.data(), oacc.data(), ostamps.data(),
                             has_pierced ? opierced.data() : nullptr, ocap, kept, d));
        written[d] += 1;
    }
    int64_t sum = 0;
    for (int c = 0; c < ACCR_REASONS; ++c) sum += counters[c];
    assert(sum == m && counters[ACCR_KEPT] == kept);
    for (int64_t d = 0; d < ocap; ++d) {
        assert(written[d] == (d < kept ? 1 : 0));
        if (d < kept) {
            assert(d == 0 || okeys[d - 1] < okeys[d]);
            continue;
        }
        assert(okeys[d] == POISON_KEY && ostamps[d] == POISON_I32 && ostamps[ocap + d] == POISON_I32);
        for (int c = 0; c < ACC_FIELDS; ++c) assert(oacc[(size_t)c * ocap + d] == POISON_ACC);
        if (has_pierced) assert(opierced[d] == POISON_I32);
    }
    wr(o, counters);
    std::vector<int64_t> k64(kept), a64((size_t)ACC_FIELDS * kept);
    std::vector<int32_t> s32(2 * kept), p32(has_pierced ? kept : 0);
    for (int64_t d = 0; d < kept; ++d) {
        k64[d] = (int64_t)okeys[d];
        for (int c = 0; c < ACC_FIELDS; ++c) a64[(size_t)c * kept + d] = oacc[(size_t)c * ocap + d];
        s32[d] = ostamps[d];
        s32[kept + d] = ostamps[ocap + d];
        if (has_pierced) p32[d] = opierced[d];
    }
    wr(o, k64); wr(o, a64); wr(o, s32); wr(o, p32); wr(o, kout); wr(o, reason);
    fclose(o);
    fclose(f);
    return 0;
}
