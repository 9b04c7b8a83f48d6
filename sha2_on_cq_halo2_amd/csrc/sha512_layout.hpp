// The SHA-512 / SHA-384 compression circuit's layout, stated once: which bit field of which 64-bit word of a region sits
// in which cell.  The synthesis kernel (sha512.hip) unrolls over this table; the constraint system
// (sha2_on_cq_halo2_amd/sha512_circuit.py) reads it through cq_sha512_layout and builds its gates, lookups and fixed
// columns from it.  The cell record, the word kinds and the forms are sha256_layout.hpp's; field meaning:
// include/cq_halo2.h, cq_sha512_layout.
#pragma once
#include <stdint.h>

#include "cq_halo2.h"
#include "sha256_layout.hpp"

namespace cq {

// a (dense, spread) pair in slot j of region row r: bits [off, off + len) of word `src`
#define SHA_PIECE(src, r, j, off, len) {CQ_SHA256_SRC_##src, CQ_SHA256_FORM_PAIR, 2 * (j), r, off, 0, len}
// chunk c of an even / odd word: bits [c * table_bits, (c + 1) * table_bits) as far as the word goes.  The chunks fill
// rows 4 .. 14 slot after slot: chunk number s of the 84 sits in slot s % 8 of row 4 + s / 8.
#define SHA_CHUNK(src, s, c) {CQ_SHA256_SRC_##src, CQ_SHA256_FORM_PAIR, 2 * ((s) % CQ_SHA256_PAIRS), 4 + (s) / CQ_SHA256_PAIRS, 0, c, 0}
#define SHA_CHUNKS(src, s) \
  SHA_CHUNK(src, s, 0), SHA_CHUNK(src, (s) + 1, 1), SHA_CHUNK(src, (s) + 2, 2), SHA_CHUNK(src, (s) + 3, 3), SHA_CHUNK(src, (s) + 4, 4), \
      SHA_CHUNK(src, (s) + 5, 5)
// decomposition d of the seven: the six chunks of its even word, then the six of its odd word
#define SHA_EVEN_ODD(src, d) SHA_CHUNKS(src##_EVEN, 2 * CQ_SHA512_CHUNKS * (d)), SHA_CHUNKS(src##_ODD, 2 * CQ_SHA512_CHUNKS * (d) + CQ_SHA512_CHUNKS)
#define SHA_WORD(src, col, r) {CQ_SHA256_SRC_##src, CQ_SHA256_FORM_WORD, col, r, 0, 0, 64}
#define SHA_SPREAD(src, col, r) {CQ_SHA256_SRC_##src, CQ_SHA256_FORM_SPREAD, col, r, 0, 0, 64}

constexpr Sha256Cell SHA512_CELLS[] = {
    // row 0: a cut at Sigma0's rotations (28, 34, 39), the 28 bits below 28 as 10 + 9 + 9, the 25 above 39 as 9 + 8 + 8
    SHA_PIECE(A, 0, 0, 0, 10), SHA_PIECE(A, 0, 1, 10, 9), SHA_PIECE(A, 0, 2, 19, 9), SHA_PIECE(A, 0, 3, 28, 6), SHA_PIECE(A, 0, 4, 34, 5),
    SHA_PIECE(A, 0, 5, 39, 9), SHA_PIECE(A, 0, 6, 48, 8), SHA_PIECE(A, 0, 7, 56, 8),
    // row 1 and slot 0 of row 2: e cut at Sigma1's rotations (14, 18, 41): 7 + 7, 4, 8 + 8 + 7, 8 + 8 + 7
    SHA_PIECE(E, 1, 0, 0, 7), SHA_PIECE(E, 1, 1, 7, 7), SHA_PIECE(E, 1, 2, 14, 4), SHA_PIECE(E, 1, 3, 18, 8), SHA_PIECE(E, 1, 4, 26, 8),
    SHA_PIECE(E, 1, 5, 34, 7), SHA_PIECE(E, 1, 6, 41, 8), SHA_PIECE(E, 1, 7, 49, 8), SHA_PIECE(E, 2, 0, 57, 7),
    // row 2: the three carries, three bits each
    SHA_PIECE(CARRY_A, 2, 1, 0, 3), SHA_PIECE(CARRY_E, 2, 2, 0, 3), SHA_PIECE(CARRY_W, 2, 3, 0, 3),
    // rows 2 and 3: W cut at sigma0's (1, 8, >> 7) and sigma1's (19, 61, >> 6) boundaries, the 42 bits between 19 and 61 as
    // 11 + 11 + 10 + 10
    SHA_PIECE(W, 2, 4, 0, 1), SHA_PIECE(W, 2, 5, 1, 5), SHA_PIECE(W, 2, 6, 6, 1), SHA_PIECE(W, 2, 7, 7, 1), SHA_PIECE(W, 3, 0, 8, 11),
    SHA_PIECE(W, 3, 1, 19, 11), SHA_PIECE(W, 3, 2, 30, 11), SHA_PIECE(W, 3, 3, 41, 10), SHA_PIECE(W, 3, 4, 51, 10), SHA_PIECE(W, 3, 5, 61, 3),
    // rows 4 .. 14: the even / odd words of Sigma0, Sigma1, Maj, the two halves of Ch, sigma0(W) and sigma1(W)
    SHA_EVEN_ODD(S0, 0), SHA_EVEN_ODD(S1, 1), SHA_EVEN_ODD(MAJ, 2), SHA_EVEN_ODD(CHP, 3), SHA_EVEN_ODD(CHQ, 4), SHA_EVEN_ODD(G0, 5),
    SHA_EVEN_ODD(G1, 6),
    // the words the additions and the copy constraints read
    SHA_WORD(A, SHA256_COL_X, 0), SHA_WORD(E, SHA256_COL_X, 1), SHA_WORD(W, SHA256_COL_X, 2), SHA_WORD(S0_EVEN, SHA256_COL_X, 3),
    SHA_WORD(S1_EVEN, SHA256_COL_X, 4), SHA_WORD(MAJ_ODD, SHA256_COL_X, 5), SHA_WORD(CH, SHA256_COL_X, 6), SHA_WORD(K, SHA256_COL_X, 7),
    SHA_SPREAD(A, SHA256_COL_Y, 0), SHA_SPREAD(E, SHA256_COL_Y, 1), SHA_WORD(G0_EVEN, SHA256_COL_Y, 2), SHA_WORD(G1_EVEN, SHA256_COL_Y, 3),
};
constexpr uint32_t SHA512_NUM_CELLS = sizeof(SHA512_CELLS) / sizeof(SHA512_CELLS[0]);
static_assert(4 + (2 * CQ_SHA512_CHUNKS * 7 - 1) / CQ_SHA256_PAIRS < CQ_SHA512_REGION_ROWS, "the chunks' rows lie inside a region");

#undef SHA_PIECE
#undef SHA_CHUNK
#undef SHA_CHUNKS
#undef SHA_EVEN_ODD
#undef SHA_WORD
#undef SHA_SPREAD

}  // namespace cq
