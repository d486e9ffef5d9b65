// The chunk arithmetic of every row upload (for_row_chunks, api_internal.h): `n` source rows become `rows_out >= n` rows
// of a device image, the rows from n on as zeros, in pieces of at most chunk_rows >= 1 source rows.  One convention for
// all callers: the pieces walk the SOURCE rows, and the piece that holds the last source row (the only piece, when
// n == 0) takes the whole zero tail with it -- it may write more than chunk_rows rows.  The pieces cover the source rows
// [0, n) and the output rows [0, rows_out) exactly once each, in order; rows_out == 0 has no piece.
// No HIP here: tests/row_chunks_main.cpp checks this file alone, on the host.
#pragma once
#include <cstdint>

namespace vscmi {

struct RowPiece {
    int64_t r0;        // first source row == first output row of the piece
    int64_t rows;      // source rows [r0, r0 + rows), <= chunk_rows
    int64_t rows_out;  // output rows [r0, r0 + rows_out) the piece writes: `rows` from the source, the rest zeros
};

// The piece that starts at row r0 (0, or the end of the piece before); the walk ends when r0 reaches rows_out
inline RowPiece row_piece(int64_t r0, int64_t n, int64_t rows_out, int64_t chunk_rows) {
    const int64_t left = n > r0 ? n - r0 : 0;
    const int64_t rows = left < chunk_rows ? left : chunk_rows;
    return {r0, rows, rows == left ? rows_out - r0 : rows};
}

}  // namespace vscmi
