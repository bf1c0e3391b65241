// abi_features.cpp -- the MFCC / LPC extractor and the LTSD voice-activity front end.
#include "abi_internal.hpp"

#include "mfcc.hpp"
#include "mfcc_plan.hpp"

#include <algorithm>
#include <cstring>

using namespace sr;

extern "C" {

SRMfcc *sr_mfcc_create(double fs, double win_length_ms, double win_shift_ms, int fft_size,
                       int n_filters, int n_ceps, double pre_emphasis) {
    SR_TRY
    return new SRMfcc(fs, win_length_ms, win_shift_ms, fft_size, n_filters, n_ceps, pre_emphasis);
    SR_CATCH(nullptr)
}

int sr_mfcc_set_lpc(SRMfcc *m, int n_lpc) {
    SR_TRY
    if (!m) fail("null extractor");
    if (n_lpc != 0 && n_lpc != 10 && n_lpc != 12 && n_lpc != 15 && n_lpc != 16 && n_lpc != 20)
        fail("LPC order %d is not instantiated (10, 12, 15, 16, 20; 0 = off)", n_lpc);
    m->n_lpc = n_lpc;
    return 0;
    SR_CATCH(-1)
}

void sr_mfcc_free(SRMfcc *m) { delete m; }
int sr_mfcc_frame_len(SRMfcc *m) { return m ? m->frame_len : 0; }
int sr_mfcc_frame_shift(SRMfcc *m) { return m ? m->frame_shift : 0; }
int64_t sr_mfcc_num_frames(SRMfcc *m, int64_t n_samples) { return m ? mfcc_num_frames(*m, n_samples) : 0; }

int sr_mfcc_tables(SRMfcc *m, double *window, double *melbank, double *dct) {
    SR_TRY
    if (!m) fail("null extractor");
    if (window) std::memcpy(window, m->window.data(), sizeof(double) * m->window.size());
    if (melbank) std::memcpy(melbank, m->melbank.data(), sizeof(double) * m->melbank.size());
    if (dct) std::memcpy(dct, m->dct.data(), sizeof(double) * m->dct.size());
    return 0;
    SR_CATCH(-1)
}

int sr_mfcc_plan(SRMfcc *m, int precision, int generic, int pcm_kind, int64_t n_frames, int n_cu, int32_t *out, int n_out) {
    SR_TRY
    if (!m || !out) fail("null argument");
    if (precision != 0 && precision != 2) fail("mfcc_precision must be 0 or 2");
    if (pcm_kind != 0 && pcm_kind != 1) fail("PCM kind: 0 = int16, 1 = float32");      // (selects the PcmT instance only: no decision hangs on it)
    if (n_out < 16) fail("sr_mfcc_plan writes 16 fields");
    n_cu = plan_n_cu(n_cu);
    const MelLayout mel = mel_layout(*m);
    const MfccPlan p = plan_mfcc(*m, mel, precision, generic != 0, n_frames, n_cu);
    const int32_t v[16] = {p.kernel, p.n1, p.nz1, p.preset, p.wpb, (int32_t)p.lds, (int32_t)std::min<int64_t>(p.frames_per_wave, INT32_MAX), p.grid, p.cp,
                           mel.pad_floats, mel.pass_len[0], mel.pass_len[1], mel.pass_len[2], mel.pass_len[3], mel.max_read, mel.n_empty};
    std::memcpy(out, v, sizeof v);
    return 16;
    SR_CATCH(-1)
}

SRBatch *sr_mfcc_extract_batch(SRMfcc *m, SRBatch *pcm, int nd, int cmvn) {
    SR_TRY
    if (!m || !pcm) fail("null argument");
    auto out = std::make_unique<SRBatch>();
    mfcc_extract_batch(*m, *pcm, nd, cmvn, *out);
    return out.release();
    SR_CATCH(nullptr)
}

int64_t sr_ltsd_num_windows(int64_t n_samples, int winsize) {
    SR_TRY
    return ltsd_num_windows(n_samples, winsize);
    SR_CATCH(-1)
}

int sr_ltsd_noise_spectrum(SRBatch *noise, int winsize, float *avg_amp_out) {
    SR_TRY
    if (!noise || !avg_amp_out) fail("null argument");
    ltsd_noise_spectrum(*noise, winsize, avg_amp_out);
    return 0;
    SR_CATCH(-1)
}

int sr_ltsd_compute(SRBatch *pcm, int winsize, int order, const float *noise_amp, float *ltsd_out,
                    int64_t *win_offsets_out) {
    SR_TRY
    if (!pcm || !noise_amp || !ltsd_out) fail("null argument");
    ltsd_compute(*pcm, winsize, order, noise_amp, ltsd_out, win_offsets_out);
    return 0;
    SR_CATCH(-1)
}

}  // extern "C"
