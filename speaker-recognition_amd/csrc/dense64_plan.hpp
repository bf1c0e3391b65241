// dense64_plan.hpp -- the float64 dense layer's decisions: the geometry of its strided GEMM (dense64.hip) and of the factorisation
// of one R x R block by one workgroup (dense64_dev.hpp), and every launch shape and LDS size that follows from them.  The layer owns
// these numbers; JFA estimation and scoring (jfa_plan.hpp), the i-vector back end (plda_plan.hpp, eig_plan.hpp) and score
// normalisation (norm_plan.hpp) plan with them and restate none.
// Host-only C++17, header-only, nothing of HIP.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>

namespace sr {

constexpr int DENSE_WG = 256;               // lanes of the layer's workgroups: the GEMM's four waves, the factorisation's loops
constexpr int DENSE_TILE = 64;              // a GEMM workgroup's output tile, 64 x 64: four waves of 16 rows x 64 columns
constexpr int DENSE_KSTEP = 16;             // reduction step of the GEMM kernel: a tile of 16 = four 16x16x4 matrix instructions
constexpr int DENSE_TS = DENSE_TILE + 4;    // row stride of the GEMM's operand tiles in LDS
constexpr int DENSE_NB = 16;                // columns of a Cholesky panel
constexpr int DENSE_PS = DENSE_NB + 1;      // row stride of the panel in LDS
constexpr int DENSE_MAX_R = 512;            // largest rank built: the factorisation's panel of DENSE_NB columns x R rows lives in LDS
constexpr int DENSE_LDS_MAX_R = 112;        // largest R x R block the whole-matrix-in-LDS path takes (112^2 x 8 B = 98 KiB + the panel)

struct Grid2 {
    int64_t x = 0, y = 0;
};

// The GEMM's grid for an output of M rows x N columns: column tiles along x, row tiles along y (at most 65535 of them).
inline Grid2 dense_gemm_grid(int64_t M, int64_t N) { return Grid2{(N + DENSE_TILE - 1) / DENSE_TILE, (M + DENSE_TILE - 1) / DENSE_TILE}; }

// Its two operand tiles [DENSE_KSTEP][DENSE_TS].
inline int dense_gemm_lds_bytes() { return 2 * DENSE_KSTEP * DENSE_TS * (int)sizeof(double); }

// What a kernel around dense_cholesky asks for: the panel [R][DENSE_PS], `vectors` work vectors [R] (2: JFA's factor and kscore
// kernels; 1: PLDA's invert kernel) and, on path 0, the block itself.
inline int dense_factor_lds_bytes(int R, int path, int vectors) {
    return (int)(((int64_t)R * DENSE_PS + vectors * (int64_t)R + (path == 0 ? (int64_t)R * R : 0)) * (int64_t)sizeof(double));
}

// Largest R the LDS path (path 0) takes for the option jfa_lds_rows (0 = automatic); above it a block is factored in place in
// global memory with its panels in LDS (path 1).
inline int dense_lds_limit(int lds_rows) { return lds_rows <= 0 ? DENSE_LDS_MAX_R : std::min(lds_rows, DENSE_LDS_MAX_R); }

// The option's range; true, or false with the text.
inline bool dense_check_lds_rows(long lds_rows, std::string &why) {
    if (lds_rows < 0 || lds_rows > DENSE_LDS_MAX_R) {
        char buf[96];
        snprintf(buf, sizeof buf, "jfa_lds_rows must be 0 (automatic) or 1 .. %d", DENSE_LDS_MAX_R);
        why = buf;
        return false;
    }
    return true;
}

}  // namespace sr
