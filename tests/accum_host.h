// Test support shared by the host drivers of the accumulated scene cloud (tests/accum*_host_driver.cpp): file reading and
// writing, the poison values, a map at its capacity with chosen values behind the rows in use, the checks on a poisoned output map, the exclusive
// scan and the row table of extract's filter.  Nothing under pcaccumulation_amd/csrc includes it.  Every function is a template or static inline:
// a driver that leaves one unused still builds under -Wall -Werror.
//   a map in a file: i64 keys[m]; i64 acc[5][m]; i32 stamps[2][m]; i32 pierced[m] (with a sidecar) -- row stride m; in memory the stride is the capacity
#pragma once
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>

#include "accum_grid.h"

typedef unsigned long long u64;

// ---- files ----------------------------------------------------------------------------------------------------------------------------------------
static inline void open_io(int argc, char **argv, FILE **f, FILE **o)
{
    assert(argc == 3);
    *f = fopen(argv[1], "rb");
    *o = fopen(argv[2], "wb");
    assert(*f && *o);
}

static inline void close_io(FILE *f, FILE *o)
{
    fclose(o);
    fclose(f);
}

template <class T> static std::vector<T> rd(FILE *f, size_t n)
{
    std::vector<T> v(n);
    if (n) assert(fread(v.data(), sizeof(T), n, f) == n);
    return v;
}

template <class T> static void wr(FILE *f, const std::vector<T> &v, size_t n)
{
    assert(n <= v.size());
    if (n) assert(fwrite(v.data(), sizeof(T), n, f) == n);
}

template <class T> static void wr(FILE *f, const std::vector<T> &v) { wr(f, v, v.size()); }

template <class T> static void wr1(FILE *f, const T &v) { assert(fwrite(&v, sizeof(T), 1, f) == 1); }

// ---- poison: what an output holds before it is written ---------------------------------------------------------------------------------------------
#define POISON_KEY 0x5a5a5a5a5a5a5a5aull
#define POISON_ACC 0x5b5b5b5b5b5b5b5bll
#define POISON_I32 0x5c5c5c5c
#define POISON_U8 0x5d
#define POISON_F32 -1234.5f
#define POISON_F64 -12345.678
#define POISON_COUNT 0x5a5a5a5a         // the ray counts behind row m (C7)
#define POISON_BYTE 0xa5                // every byte of every output column of C9 and C10, whatever its type

template <class T> static bool is_poison(const T &v)
{
    unsigned char b[sizeof(T)];
    memcpy(b, &v, sizeof(T));
    for (size_t k = 0; k < sizeof(T); ++k)
        if (b[k] != POISON_BYTE) return false;
    return true;
}

template <class T> static std::vector<T> poisoned(size_t n)
{
    std::vector<T> v(n);
    if (n) memset(v.data(), POISON_BYTE, n * sizeof(T));
    return v;
}

// ---- a map -----------------------------------------------------------------------------------------------------------------------------------------
struct Map {
    int64_t m, cap;
    bool has_pierced;
    std::vector<u64> keys;
    std::vector<int64_t> acc;                                                    // [ACC_FIELDS][cap]
    std::vector<int32_t> stamps, pierced;                                        // [2][cap], [cap]
    const int32_t *p() const { return has_pierced ? pierced.data() : nullptr; }
    int32_t *p() { return has_pierced ? pierced.data() : nullptr; }
};

// What the rows behind m hold.  A stray read of them must not fail where it could be told from a valid one, so each driver picks values that pass
// its own filters: `moving` is field 1 of acc, `acc` every other field.
struct Fills {
    u64 key;
    int64_t acc, moving;
    int32_t stamp, pierced;
};

enum { MAP_ACC = 1, MAP_STAMPS = 2 };

// Reads m rows from where the file stands into tables of `cap` rows; `parts` names the tables the file holds besides the keys (the others stay empty).
static inline Map read_map(FILE *f, int64_t m, int64_t cap, bool has_pierced, const Fills &fills, int parts = MAP_ACC | MAP_STAMPS)
{
    assert(m >= 0 && cap >= m && cap >= 1);
    const bool has_acc = (parts & MAP_ACC) != 0, has_stamps = (parts & MAP_STAMPS) != 0;
    Map t;
    t.m = m; t.cap = cap; t.has_pierced = has_pierced;
    t.keys.assign(cap, fills.key);
    t.acc.assign(has_acc ? (size_t)ACC_FIELDS * cap : 0, fills.acc);
    for (int64_t i = m; has_acc && i < cap; ++i) t.acc[accum_field(1, i, cap)] = fills.moving;
    t.stamps.assign(has_stamps ? 2 * cap : 0, fills.stamp);
    t.pierced.assign(has_pierced ? cap : 0, fills.pierced);
    const std::vector<int64_t> k = rd<int64_t>(f, m), a = rd<int64_t>(f, has_acc ? (size_t)ACC_FIELDS * m : 0);
    const std::vector<int32_t> s = rd<int32_t>(f, has_stamps ? 2 * m : 0), p = rd<int32_t>(f, has_pierced ? m : 0);
    for (int64_t i = 0; i < m; ++i) {
        t.keys[i] = (u64)k[i];
        assert(i == 0 || t.keys[i - 1] < t.keys[i]);
        for (int c = 0; has_acc && c < ACC_FIELDS; ++c) t.acc[(size_t)c * cap + i] = a[(size_t)c * m + i];
        if (has_stamps) { t.stamps[i] = s[i]; t.stamps[cap + i] = s[m + i]; }
        if (has_pierced) t.pierced[i] = p[i];
    }
    return t;
}

static inline Map poison_map(int64_t cap, bool has_pierced)
{
    Map t;
    t.m = 0; t.cap = cap; t.has_pierced = has_pierced;
    t.keys.assign(cap, POISON_KEY);
    t.acc.assign((size_t)ACC_FIELDS * cap, POISON_ACC);
    t.stamps.assign(2 * cap, POISON_I32);
    t.pierced.assign(has_pierced ? cap : 0, POISON_I32);
    return t;
}

// The rows of a poisoned map from `row` on are still poison.
static inline void assert_poison_from(const Map &t, int64_t row)
{
    for (int64_t d = row; d < t.cap; ++d) {
        assert(t.keys[d] == POISON_KEY && t.stamps[d] == POISON_I32 && t.stamps[t.cap + d] == POISON_I32);
        for (int c = 0; c < ACC_FIELDS; ++c) assert(t.acc[(size_t)c * t.cap + d] == POISON_ACC);
        if (t.has_pierced) assert(t.pierced[d] == POISON_I32);
    }
}

// written[d] counts the stores to destination d: once below `rows`, never behind.
static inline void assert_written_once(const std::vector<int> &written, int64_t rows)
{
    for (size_t d = 0; d < written.size(); ++d) assert(written[d] == ((int64_t)d < rows ? 1 : 0));
}

// The first `rows` rows, keys ascending, at row stride.
static inline void write_map(FILE *o, const Map &t, int64_t rows)
{
    std::vector<int64_t> k64(rows), a64((size_t)ACC_FIELDS * rows);
    std::vector<int32_t> s32(2 * rows), p32(t.has_pierced ? rows : 0);
    for (int64_t d = 0; d < rows; ++d) {
        assert(d == 0 || t.keys[d - 1] < t.keys[d]);
        k64[d] = (int64_t)t.keys[d];
        for (int c = 0; c < ACC_FIELDS; ++c) a64[(size_t)c * rows + d] = t.acc[(size_t)c * t.cap + d];
        s32[d] = t.stamps[d];
        s32[rows + d] = t.stamps[t.cap + d];
        if (t.has_pierced) p32[d] = t.pierced[d];
    }
    wr(o, k64); wr(o, a64); wr(o, s32); wr(o, p32);
}

// ---- scan and row table ----------------------------------------------------------------------------------------------------------------------------
// out[0..n] = exclusive scan of flag, out[n] = total
static inline std::vector<int> scan(const std::vector<int> &flag)
{
    std::vector<int> out(flag.size() + 1, 0);
    for (size_t i = 0; i < flag.size(); ++i) out[i + 1] = out[i] + flag[i];
    return out;
}

// The rows a flag keeps, in order: dst[i] = the kept row of map row i or -1, rows[j] = the map row of kept row j.
struct RowTable {
    std::vector<int> keep, kpos, dst, rows;
    int64_t kept;
};

static inline RowTable row_table(const std::vector<int> &keep)
{
    const int64_t m = (int64_t)keep.size();
    RowTable t;
    t.keep = keep;
    t.kpos = scan(keep);
    t.kept = t.kpos[m];
    t.dst.assign(m, -1);
    t.rows.assign(t.kept, -1);
    for (int64_t i = 0; i < m; ++i) {
        if (!keep[i]) continue;
        const int64_t d = accum_merge_dst(t.kpos[i], 0, t.kept);
        assert(d >= 0);
        PCACC_BOUND(d, t.kept);
        assert(t.rows[d] == -1);
        t.dst[i] = (int)d;
        t.rows[d] = (int)i;
    }
    return t;
}

// Pass 1 of C5: the keep flags of extract's predicate, then the table.
static inline RowTable row_table(const Map &t, int64_t min_count, bool use_fraction, double fraction)
{
    std::vector<int> keep(t.m);
    for (int64_t i = 0; i < t.m; ++i)
        keep[i] = accum_keep(t.acc[accum_field(0, i, t.cap)], t.acc[accum_field(1, i, t.cap)], min_count, use_fraction, fraction) ? 1 : 0;
    return row_table(keep);
}
