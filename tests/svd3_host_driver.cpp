// Host build of pcaccumulation_amd/csrc/svd3.h (tests/test_ego_solve.py): the 3x3 SVD that ego_kabsch_kernel and svd3_kernel call, run on the CPU
// in float64 so that its factors can be held to the bounds of double arithmetic against LAPACK.
//   in : i64 n, then n row-major 3x3 matrices as f64
//   out: per matrix 21 f64: u[9], s[3], v[9] (row-major)
// Exit status 0 only when everything was read and written.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "svd3.h"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: svd3_host_driver <in.bin> <out.bin>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int64_t n = 0;
    if (fread(&n, 8, 1, f) != 1 || n < 0) { fprintf(stderr, "bad header\n"); return 1; }
    std::vector<double> in(9 * n), out(21 * n);
    if (n && fread(in.data(), 8, 9 * n, f) != (size_t)(9 * n)) { fprintf(stderr, "short input\n"); return 1; }
    fclose(f);
    for (int64_t m = 0; m < n; ++m) {
        double a[3][3], u[3][3], s[3], v[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) a[i][j] = in[9 * m + 3 * i + j];
        jacobi_svd3(a, u, s, v);
        for (int i = 0; i < 3; ++i) {
            out[21 * m + 9 + i] = s[i];
            for (int j = 0; j < 3; ++j) { out[21 * m + 3 * i + j] = u[i][j]; out[21 * m + 12 + 3 * i + j] = v[i][j]; }
        }
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 1; }
    if (n && fwrite(out.data(), 8, 21 * n, o) != (size_t)(21 * n)) { fprintf(stderr, "short write\n"); return 1; }
    if (fclose(o) != 0) { perror(argv[2]); return 1; }
    return 0;
}
