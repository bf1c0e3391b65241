// jfa.hpp -- statistics handles and JFA on the device, host entry points: jfa_stats.hip, jfa.hip, jfa_score.hip.  The handle types
// and what those files hand each other are in jfa_dev.hpp.
#pragma once

#include <cstdint>

struct SRJfa;
struct SRStats;

namespace sr {

// jfa_stats.hip: the life of a statistics handle (bw_stats.hpp: bw_stats_resident fills one).  Every refusal comes before any device
// work.
SRStats *stats_from_host(int64_t n, int K, int D, const double *N, const double *F);
void stats_info(const SRStats *s, int64_t *out, int n_out);
void stats_get(const SRStats *s, double *N, double *F);
SRStats *stats_take(const SRStats *s, const int64_t *rows, int64_t n_rows);
void stats_close(SRStats *s);
// jfa_stats.hip: grouping and centring on the device into a factor handle, what it holds, the z / d iteration on it, and the two
// scorers on a statistics handle (jfa_plan.hpp has the formulas).
SRJfa *jfa_open_centred(const SRStats *s, const double *E, const double *m, int mode, const int64_t *ids, int64_t n_labels, const double *d,
                        const double *z, const double *v, int Ry, const double *y, const double *u, int Ru, const double *x);
void jfa_statistics(SRJfa &h, double *N, double *Fc);
void jfa_zd(SRJfa &h, double *d, int n_iter, double *z, double *a, double *b);
void jfa_score_stats(int mode, const SRStats *tst, int64_t J, int Ry, int Ru, const double *m, const double *E, const double *d, const double *v,
                     const double *u, const double *z, const double *y, const double *x, const unsigned char *mask, int64_t mask_rows,
                     int64_t mask_cols, double *out, int64_t *empty_segments, int64_t *bad_segments);
// jfa.hip: JFA factor estimation on resident statistics (eigenvoices, eigenchannels; jfa_plan.hpp has the formulas).  Every
// refusal (jfa_plan.cpp) comes before any device work.  Host pointers throughout; W [R][K D] in / out where it says so.
SRJfa *jfa_open(int64_t G, int K, int D, const double *N, const double *Fc, const double *E);
void jfa_factors(SRJfa &h, const double *W, int R, double *y, double *A, double *C, int64_t *bad_groups);
void jfa_update(int K, int D, int R, const double *A, const double *C, double *W, int64_t *skipped);
void jfa_train(SRJfa &h, double *W, int R, int n_iter, double *y, int64_t *skipped);
void jfa_close(SRJfa *h);
// jfa_score.hip: the score matrix out [J][T] of J models against T test segments, mode 0 integrated (kscore_famous_19.m), 1 linear
// (linear_scoring.m; needs x).  d, z, x, mask: null = absent.  Every refusal (jfa_plan.cpp) comes before any device work.
void jfa_score(int mode, int64_t T, int64_t J, int K, int D, int Ry, int Ru, const double *N, const double *F, const double *m, const double *E,
               const double *d, const double *v, const double *u, const double *z, const double *y, const double *x, const unsigned char *mask,
               int64_t mask_rows, int64_t mask_cols, double *out, int64_t *empty_segments, int64_t *bad_segments);
void set_jfa_scratch_mib(long v);
long jfa_scratch_mib();
void set_jfa_lds_rows(long v);
long jfa_lds_rows();

}  // namespace sr
