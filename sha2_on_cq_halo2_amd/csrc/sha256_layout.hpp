// The SHA-256 compression circuit's layout, stated once: which bit field of which 32-bit word of a region sits in
// which cell.  The synthesis kernel (sha256.hip) unrolls over this table; the constraint system
// (sha2_on_cq_halo2_amd/sha256_circuit.py) reads it through cq_sha256_layout and builds its gates, lookups and fixed
// columns from it.  Field meaning: include/cq_halo2.h, cq_sha256_layout.
#pragma once
#include <stdint.h>

#include "cq_halo2.h"

namespace cq {

struct Sha256Cell {
  uint32_t kind, form, column, row, offset, per_table_bits, len;
};

// a (dense, spread) pair in slot j of region row r: bits [off, off + len) of word `src`
#define SHA_PIECE(src, r, j, off, len) {CQ_SHA256_SRC_##src, CQ_SHA256_FORM_PAIR, 2 * (j), r, off, 0, len}
// chunk c of an even / odd word: bits [c * table_bits, (c + 1) * table_bits) as far as the word goes
#define SHA_CHUNK(src, r, j, c) {CQ_SHA256_SRC_##src, CQ_SHA256_FORM_PAIR, 2 * (j), r, 0, c, 0}
// the three chunks of the even word in slots 0..2 of row r, those of the odd word in slots 3..5
#define SHA_EVEN_ODD(src, r)                                                                               \
  SHA_CHUNK(src##_EVEN, r, 0, 0), SHA_CHUNK(src##_EVEN, r, 1, 1), SHA_CHUNK(src##_EVEN, r, 2, 2),            \
      SHA_CHUNK(src##_ODD, r, 3, 0), SHA_CHUNK(src##_ODD, r, 4, 1), SHA_CHUNK(src##_ODD, r, 5, 2)
#define SHA_WORD(src, col, r) {CQ_SHA256_SRC_##src, CQ_SHA256_FORM_WORD, col, r, 0, 0, 32}
#define SHA_SPREAD(src, col, r) {CQ_SHA256_SRC_##src, CQ_SHA256_FORM_SPREAD, col, r, 0, 0, 32}

constexpr uint32_t SHA256_COL_X = 2 * CQ_SHA256_PAIRS, SHA256_COL_Y = 2 * CQ_SHA256_PAIRS + 1;

constexpr Sha256Cell SHA256_CELLS[] = {
    // row 0: a cut at Sigma0's rotations (2, 13, 22); the three carries, three bits each
    SHA_PIECE(A, 0, 0, 0, 2), SHA_PIECE(A, 0, 1, 2, 11), SHA_PIECE(A, 0, 2, 13, 9), SHA_PIECE(A, 0, 3, 22, 10),
    SHA_PIECE(CARRY_A, 0, 4, 0, 3), SHA_PIECE(CARRY_E, 0, 5, 0, 3), SHA_PIECE(CARRY_W, 0, 6, 0, 3),
    // row 1: e cut at Sigma1's rotations (6, 11, 25), the 14 bits between 11 and 25 halved
    SHA_PIECE(E, 1, 0, 0, 6), SHA_PIECE(E, 1, 1, 6, 5), SHA_PIECE(E, 1, 2, 11, 7), SHA_PIECE(E, 1, 3, 18, 7), SHA_PIECE(E, 1, 4, 25, 7),
    // row 2: W cut at sigma0's (7, 18, >> 3) and sigma1's (17, 19, >> 10) boundaries, the 13 bits above 19 as 7 + 6
    SHA_PIECE(W, 2, 0, 0, 3), SHA_PIECE(W, 2, 1, 3, 4), SHA_PIECE(W, 2, 2, 7, 3), SHA_PIECE(W, 2, 3, 10, 7), SHA_PIECE(W, 2, 4, 17, 1),
    SHA_PIECE(W, 2, 5, 18, 1), SHA_PIECE(W, 2, 6, 19, 7), SHA_PIECE(W, 2, 7, 26, 6),
    // rows 3 .. 7: the even / odd words of Sigma0, Sigma1, Maj and the two halves of Ch
    SHA_EVEN_ODD(S0, 3), SHA_EVEN_ODD(S1, 4), SHA_EVEN_ODD(MAJ, 5), SHA_EVEN_ODD(CHP, 6), SHA_EVEN_ODD(CHQ, 7),
    // sigma0(W) and sigma1(W) in the slots those rows leave
    SHA_CHUNK(G0_EVEN, 3, 6, 0), SHA_CHUNK(G0_ODD, 3, 7, 0), SHA_CHUNK(G0_EVEN, 4, 6, 1), SHA_CHUNK(G0_ODD, 4, 7, 1),
    SHA_CHUNK(G0_EVEN, 5, 6, 2), SHA_CHUNK(G0_ODD, 5, 7, 2), SHA_CHUNK(G1_EVEN, 6, 6, 0), SHA_CHUNK(G1_ODD, 6, 7, 0),
    SHA_CHUNK(G1_EVEN, 7, 6, 1), SHA_CHUNK(G1_ODD, 7, 7, 1), SHA_CHUNK(G1_EVEN, 1, 5, 2), SHA_CHUNK(G1_ODD, 1, 6, 2),
    // the words the additions and the copy constraints read
    SHA_WORD(A, SHA256_COL_X, 0), SHA_WORD(E, SHA256_COL_X, 1), SHA_WORD(W, SHA256_COL_X, 2), SHA_WORD(S0_EVEN, SHA256_COL_X, 3),
    SHA_WORD(S1_EVEN, SHA256_COL_X, 4), SHA_WORD(MAJ_ODD, SHA256_COL_X, 5), SHA_WORD(CH, SHA256_COL_X, 6), SHA_WORD(K, SHA256_COL_X, 7),
    SHA_SPREAD(A, SHA256_COL_Y, 0), SHA_SPREAD(E, SHA256_COL_Y, 1), SHA_WORD(G0_EVEN, SHA256_COL_Y, 2), SHA_WORD(G1_EVEN, SHA256_COL_Y, 3),
};
constexpr uint32_t SHA256_NUM_CELLS = sizeof(SHA256_CELLS) / sizeof(SHA256_CELLS[0]);

#undef SHA_PIECE
#undef SHA_CHUNK
#undef SHA_EVEN_ODD
#undef SHA_WORD
#undef SHA_SPREAD

}  // namespace cq
