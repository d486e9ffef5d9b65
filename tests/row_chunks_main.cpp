// Stand-alone check of the chunk arithmetic of the row uploads (vsc2022_amd/csrc/row_chunks.h, the one header this file
// includes from the library): tests/test_row_chunks_host.py compiles it with the host compiler and the address and
// undefined-behaviour sanitizers and runs it.  Exit status 0: every property held.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "row_chunks.h"

using vscmi::RowPiece;
using vscmi::row_piece;

static int failures = 0;
#define CHECK(cond)                                                                                                       \
    do {                                                                                                                  \
        if (!(cond)) {                                                                                                    \
            if (++failures <= 20)                                                                                         \
                std::printf("n=%lld rows_out=%lld chunk_rows=%lld: %s\n", (long long)n, (long long)rows_out, (long long)chunk_rows, #cond); \
        }                                                                                                                 \
    } while (0)

// The walk as for_row_chunks makes it.  `mark`: brute-force marking arrays of the source and the output rows (small
// sizes), or nullptr (64-bit sizes: the same properties from the pieces' bounds alone).
static void walk(int64_t n, int64_t rows_out, int64_t chunk_rows, bool mark) {
    std::vector<int> src(mark ? (size_t)n : 0, 0), out(mark ? (size_t)rows_out : 0, 0);
    int64_t pieces = 0, src_next = 0;
    for (int64_t r0 = 0; r0 < rows_out;) {
        const RowPiece p = row_piece(r0, n, rows_out, chunk_rows);
        ++pieces;
        CHECK(p.r0 == r0);                           // in order, no gap, no overlap: a piece starts where the last one ended
        CHECK(p.rows >= 0 && p.rows <= chunk_rows);  // no piece has more than chunk_rows source rows
        CHECK(p.rows_out >= p.rows && p.rows_out > 0);
        CHECK(p.r0 + p.rows <= n && p.r0 + p.rows_out <= rows_out);
        CHECK(p.rows == 0 || p.r0 == src_next);      // the source rows of a piece are its first output rows
        // the zero tail belongs to the piece with the last source row (the only piece when there is no source row)
        CHECK(p.rows_out == p.rows || p.r0 + p.rows == n);
        CHECK(p.rows > 0 || n == 0);
        if (p.r0 + p.rows > n || p.r0 + p.rows_out > rows_out || p.rows_out <= 0) return;  // (would run off the arrays, or never end)
        if (mark) {
            for (int64_t r = p.r0; r < p.r0 + p.rows; ++r) ++src[(size_t)r];
            for (int64_t r = p.r0; r < p.r0 + p.rows_out; ++r) ++out[(size_t)r];
        }
        src_next = p.r0 + p.rows;
        r0 += p.rows_out;
        if (r0 == rows_out) CHECK(src_next == n);  // the walk ends with every source row handed out
    }
    CHECK(src_next == n);
    CHECK((pieces >= 1) == (rows_out > 0));  // at least one piece whenever there is a row to write, n == 0 included
    CHECK(pieces == (n == 0 ? (rows_out > 0 ? 1 : 0) : (n + chunk_rows - 1) / chunk_rows));
    for (size_t r = 0; r < src.size(); ++r) CHECK(src[r] == 1);  // covered exactly once
    for (size_t r = 0; r < out.size(); ++r) CHECK(out[r] == 1);
}

int main() {
    int64_t cases = 0;
    for (int64_t n = 0; n <= 40; ++n)
        for (int64_t rows_out = n; rows_out <= n + 12; ++rows_out)
            for (int64_t chunk_rows = 1; chunk_rows <= 17; ++chunk_rows, ++cases) walk(n, rows_out, chunk_rows, true);
    // around 2^31 rows: nothing in the arithmetic is 32 bits wide
    const int64_t G = (int64_t)1 << 31;
    const int64_t big[][3] = {{G, G + 128, 262144},         {G - 1, G + 127, G - 1},   {G + 1, G + 1, G},         {G + 5, G + 133, 1 << 20},
                              {3 * G + 7, 3 * G + 64, G + 3}, {G, G, 1 << 19},           {0, G + 64, 1},            {G + 64, G + 64, (int64_t)1 << 40},
                              {(int64_t)1 << 40, ((int64_t)1 << 40) + 192, (int64_t)1 << 27}};
    for (const auto& b : big) walk(b[0], b[1], b[2], false), ++cases;
    if (failures) {
        std::printf("row_chunks: %d property failures\n", failures);
        return 1;
    }
    std::printf("row_chunks ok: %lld cases\n", (long long)cases);
    return 0;
}
