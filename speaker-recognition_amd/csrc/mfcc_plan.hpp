// mfcc_plan.hpp -- what the MFCC stage decides before it touches the device: the padded mel-table layout of an extractor
// (mel_layout) and kernel, template arguments, workgroup shape, LDS size, frames per wave and grid of one pass over a batch
// (plan_mfcc), as pure functions of the extractor's host tables, the options, the frame count and the CU count.  Host-only
// C++17: mfcc_plan.cpp calls nothing of HIP; upload_tables, mfcc_extract_with and mfcc_launch_f64 consume what it returns, and
// tests/host/host_checks.cpp (mode "mfcc") pins the decisions on the CPU.
#pragma once

#include "mfcc.hpp"

#include <vector>

namespace sr {

constexpr int MFCC_DCT_LD = 80;     // row stride of the zero-padded DCT table in LDS: 320 B = 64 B mod 256, so the 4 rows x 4
                                    // parts of a 16-lane ds_read_b128 phase cover 16 distinct 16-byte windows (64 floats would put
                                    // all 16 rows on the same banks)
constexpr int WAVE_SLAB_C = 1088;   // complex slots per wave: max(16*68, 64*17, 1024)
constexpr int MFCC_PBUF_FLOATS = 1100;           // a wave's power-spectrum region: what a padded mel sweep may read
constexpr int MFCC_LDS_BYTES = 160 * 1024;       // LDS of a CU
constexpr int MFCC_WPB = 12;                     // waves per workgroup of the fp32 FFT-2048 kernel (4: long frames, wide banks)
constexpr int F64_WIN_BYTES = 4160;              // 520 float64 window taps in LDS (frames of <= 512 samples)
constexpr int F64_WPB = 8;                       // waves per workgroup: 8 x 17 KB of exchange slab + the mel table fill a CU's LDS

// Mel sweep lengths (16-bin steps per pass of 16 bands) of the reference's default filterbank, known at
// compile time so that the sweep unrolls completely and its LDS reads are issued ahead of their use;
// preset 0 takes the lengths from MelRuns at run time (any other fs / n_filters).
__host__ __device__ constexpr int mel_preset_steps(int preset, int pass) {
    return preset == 1 ? (pass == 0 ? 2 : pass == 1 ? 3 : pass == 2 ? 6 : 7)      // fs 16 kHz, 50 filters, FFT 2048
                       : 0;
}
constexpr int MEL_PRESETS = 1;      // presets 1..MEL_PRESETS are instantiated

// cmvn_delta_kernel: thread = (stripe of frames, coefficient), the coefficients padded to this many columns
__host__ __device__ constexpr int cmvn_col_pad(int n_ceps) { return n_ceps <= 16 ? 16 : n_ceps <= 32 ? 32 : 64; }

// The mel filterbank as the kernels read it: CSR of the nonzero weights (generic kernels) and the padded re-layout of the fast
// kernels -- pass ps holds bands 16ps..16ps+15, every run of a pass zero-padded to pass_len[ps] columns from the band's sweep start.
struct MelLayout {
    std::vector<int> row, col;      // CSR: band b's nonzero columns are col[row[b] .. row[b + 1])
    int cnt[64] = {0};              // nonzero columns of band b
    int first[64] = {0};            // its first nonzero column (0 for an empty band)
    int start[64] = {0};            // where its padded sweep starts (a multiple of 4, <= first)
    int pass_len[4] = {0, 0, 0, 0}, pass_base[4] = {0, 0, 0, 0};
    int pad_floats = 0, max_cnt = 0, nnz = 0;
    bool runs_contiguous = true;    // every band one contiguous run, every padded sweep inside MFCC_PBUF_FLOATS: the fast kernels apply
    int max_read = 0;               // largest float index of the power-spectrum region a padded sweep reads
    int n_empty = 0;                // bands without a nonzero weight (the reference takes ln 0 there)
    // float index of element e of band b's padded run in the padded table
    size_t pad_index(int b, int e) const {
        return (size_t)pass_base[b / 16] + (size_t)(e >> 4) * 256 + ((size_t)(b % 16) * 4 + ((e >> 2) & 3)) * 4 + (e & 3);
    }
};
MelLayout mel_layout(const SRMfcc &m);
// Sweep starts of the MFCC kernels' mel gather (mfcc.hip: four lanes per band, one ds_read_b128 each per step, bands {0,3,5,6},
// {1,2,4,7}, {8,11,13,14}, {9,10,12,15} of a pass of 16 served together over 16 slots of 16 bytes): start[b] <= col0[b], a multiple
// of 4, >= 0, moved down only as far as the band's padded run still fits pass_len[b / 16]; per group the choice with the fewest extra
// LDS cycles, then the least padding.  Host-only.
void mel_sweep_starts(const int *col0, const int *cnt, int n_bands, const int pass_len[4], int *start);
int mel_sweep_extra_cycles(const int *start, const int *cnt, int n_bands, int pass);      // extra LDS cycles per read instruction of that pass

enum MfccKernel { MFCC_F32_FAST = 0, MFCC_F32_GENERIC = 1, MFCC_F64_FAST = 2, MFCC_F64_GENERIC = 3 };

struct MfccPlan {
    int kernel = MFCC_F32_GENERIC;
    int n1 = 0;                     // fast kernels: complex points / 64 (template argument N1; 16 for the float64 one)
    int nz1 = 0;                    // fp32 fast kernel: the instantiated NZ1 (rows of samples); float64 fast: 4
    int preset = 0;                 // fast kernels: mel preset (template argument MP)
    int wpb = 4;                    // waves per workgroup
    size_t lds = 0;                 // dynamic LDS bytes, as launched
    int64_t frames_per_wave = 1;    // fast kernels: the contiguous frame range of a wave
    int grid = 0;
    int cp = 16;                    // cmvn_delta_kernel's column padding
};
// precision: 2 = float64 spectrum, 0 = fp32 throughout; n_frames > 0
MfccPlan plan_mfcc(const SRMfcc &m, const MelLayout &mel, int precision, bool force_generic, int64_t n_frames, int n_cu);

}  // namespace sr
