// Host build of pcaccumulation_amd/csrc/accum_prune.h (tests/test_accumulate_prune.py): the reason of a row, the neighbour count of a survivor and the
// move of a surviving row -- the functions the kernels of accum_prune.hip call -- run on the CPU with every table index assert-checked
// (-DPCACC_HOST_CHECK), before anything runs on a GPU.  The steps between them (flags, exclusive scan, dst / rows, second scan) are the kernels' steps.
// The input tables stand at their capacity with poison behind row m that no result may depend on; the output tables are poison everywhere before
// the compaction: every destination below `kept` is written exactly once, keys ascend, and the poison behind row `kept` is untouched.
//   in : i64 m, in_capacity, out_capacity, has_pierced, min_count, use_fraction, use_stamp, before_stamp, use_box, lo[3], hi[3], min_pierced, use_ratio,
//        min_neighbors, radius; f64 max_moving_fraction, ratio; a map (see accum_host.h)
//   out: i64 counters[6]; the map of `kept` rows; i32 k[m] (stage B's count of a stage-A survivor, else -1); u8 reason[m]
#include "accum_prune.h"
#include "accum_host.h"

int main(int argc, char **argv)
{
    FILE *f, *o;
    open_io(argc, argv, &f, &o);
    const std::vector<int64_t> h = rd<int64_t>(f, 19);
    const std::vector<double> g = rd<double>(f, 2);
    const int64_t m = h[0], cap = h[1], ocap = h[2];
    const bool has_pierced = h[3] != 0;
    AccrParams P;
    P.min_count = h[4]; P.use_fraction = h[5] != 0; P.use_stamp = h[6] != 0; P.before_stamp = (int32_t)h[7]; P.use_box = h[8] != 0;
    P.lo_x = (int32_t)h[9]; P.lo_y = (int32_t)h[10]; P.lo_z = (int32_t)h[11]; P.hi_x = (int32_t)h[12]; P.hi_y = (int32_t)h[13]; P.hi_z = (int32_t)h[14];
    P.min_pierced = (int32_t)h[15]; P.use_ratio = h[16] != 0; P.max_moving_fraction = g[0]; P.ratio = g[1];
    const int min_neighbors = (int)h[17], radius = (int)h[18];
    assert(ocap >= m && ocap >= 1 && min_neighbors >= 0 && min_neighbors <= ACCR_MAX_NEIGHBORS);
    assert(min_neighbors == 0 || (radius >= 1 && radius <= ACCN_MAX_RADIUS));
    // rows past m: a key that would mislead any search that read it, a record that passes every filter
    const Map in = read_map(f, m, cap, has_pierced, Fills{0, 1000, 1000, 0x7fffffff, 0});

    // stage A
    std::vector<int> flag(m);
    std::vector<uint8_t> reason(m);
    for (int64_t i = 0; i < m; ++i) {
        const int r = accr_row_reason(in.keys.data(), in.acc.data(), in.stamps.data(), in.p(), cap, m, i, P);
        assert(r >= ACCR_KEPT && r <= ACCR_PIERCED);
        flag[i] = r == ACCR_KEPT;
        reason[i] = (uint8_t)r;
    }
    // stage B
    std::vector<int32_t> kout(m, -1);
    if (min_neighbors > 0) {
        const RowTable alive = row_table(flag);
        for (int64_t j = 0; j < alive.kept; ++j) {
            const int64_t i = alive.rows[j];
            assert(i >= 0 && i < m && alive.dst[i] == j);
            const int k = accr_neighbors(in.keys.data(), m, alive.dst.data(), i, radius);
            assert(k >= 1 && k <= (2 * radius + 1) * (2 * radius + 1) * (2 * radius + 1));
            kout[i] = k;
            if (k < min_neighbors) { flag[i] = 0; reason[i] = ACCR_ISOLATED; }
        }
    }
    // compaction
    const std::vector<int> kpos = scan(flag);
    const int64_t kept = kpos[m];
    Map out = poison_map(ocap, has_pierced);
    std::vector<int> written(ocap, 0);
    std::vector<int64_t> counters(ACCR_REASONS, 0);
    for (int64_t i = 0; i < m; ++i) {
        counters[reason[i]] += 1;
        if (!flag[i]) continue;
        const int64_t d = accum_merge_dst(kpos[i], 0, kept);
        assert(d >= 0 && d < kept);
        assert(accr_move_row(in.keys.data(), in.acc.data(), in.stamps.data(), in.p(), cap, m, i, out.keys.data(), out.acc.data(), out.stamps.data(), out.p(),
                             ocap, kept, d));
        written[d] += 1;
    }
    int64_t sum = 0;
    for (int c = 0; c < ACCR_REASONS; ++c) sum += counters[c];
    assert(sum == m && counters[ACCR_KEPT] == kept);
    assert_written_once(written, kept);
    assert_poison_from(out, kept);
    wr(o, counters);
    write_map(o, out, kept);
    wr(o, kout); wr(o, reason);
    close_io(f, o);
    return 0;
}
