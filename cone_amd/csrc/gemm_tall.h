// The tall form of the row GEMM (gemm_tall.hip) and what gemm.hip's dispatcher and api.hip need of it.
#pragma once

#include "common.h"

namespace cone {

// A tile family beside common.h's GEMM_AUTO .. GEMM_ROWS8: forces the tall form (an ineligible launch is refused by name).
constexpr int GEMM_TALL = 4;

// GemmArgs::variant carries the family in its low byte.  Bits 8 and up of an automatic launch may carry the row threshold of
// the tall form for this launch (the model option "gemm_tall_min_rows"): 0 = the built-in value (CONE_GEMM_TALL_MIN_ROWS),
// 1 = the tall form is off, t + 1 = launches of at least t rows (host bound) take it.
constexpr int GEMM_VARIANT_MASK = 0xff, GEMM_TALL_MIN_SHIFT = 8, GEMM_TALL_MIN_MAX = 1 << 22;

// Automatic launches with N == 768 and at least this many rows (host-known bound) take the tall form; 0: never.  Measured
// (profiles/gemm_tall_measured.txt, tools/gemm_qkv_bench.py, the forms alternating in one process): at N = 768 the tall form
// beats the shipped forms by more than the spread of their own repeats from 262 144 rows on in every run (from 65 536 in one
// of two); at N = 256 -- 8 chunks per tile against 24 for the same per-tile costs -- it loses at every swept row count, so
// the built-in rule takes N = 768 only.  A threshold set per launch (GEMM_TALL_MIN_SHIFT) applies to every N the form runs.
#ifndef CONE_GEMM_TALL_MIN_ROWS
#define CONE_GEMM_TALL_MIN_ROWS 262144
#endif
static inline bool gemm_tall_builtin_rule(int M, int N) { return CONE_GEMM_TALL_MIN_ROWS > 0 && N == 768 && M >= CONE_GEMM_TALL_MIN_ROWS; }

// null: the tall form runs this launch; else what it cannot take, by name
const char* gemm_tall_refusal(const GemmArgs& a);
// n_cu: the CU count that sizes the persistent grid (0: the device's)
int launch_gemm_tall(const GemmArgs& a, int n_cu, hipStream_t s);

}  // namespace cone
