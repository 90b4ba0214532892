// Launch bounds of the [queries, entities] sweeps that keep no [B, N] tensor (rank.hip, bce.hip on the row GEMM; transe_1n.hip).
#pragma once
#include <stdint.h>

namespace mrg {

constexpr int64_t RANK_CHUNK = 8192;          // queries per sweep launch: bounds the [chunk, D] operands of the workspace and grid.x
constexpr int RANK_NT = 7;                    // column tiles per block of the row GEMM's sweep
constexpr int64_t RANK_MAX_N = 65535LL * RANK_NT * 32;     // grid.y
constexpr int64_t BCE_COLS = (int64_t)RANK_NT * 32 * 128;      // entity columns per sweep launch (28 672): bounds the split table

}  // namespace mrg
