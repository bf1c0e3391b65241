// ref_rand.hpp -- the reference's random numbers.  Every draw of the reference comes from libc rand() or from a
// std::default_random_engine seeded by rand() (random.hh:17-56), and rand() starts from its default seed in a fresh process.  The
// same draws are made here, in the same order, from the same generators: libstdc++'s engine and distribution, and glibc's rand()
// -- restated, because the process-wide one cannot be used: the HIP runtime draws from it while it initialises
// (scripts/debug/randcheck.py).  One restated generator is library-wide, as the reference's is process-wide; a caller who passes a
// seed gets a stream of its own.
// Host-only C++17, nothing of HIP: tests/host/kmeans_checks.cpp runs it under the host sanitizers.
#pragma once

#include <cstdint>
#include <limits>
#include <random>

namespace sr {

// random.hh:17-56
struct RefRandom {
    std::default_random_engine generator;
    std::uniform_real_distribution<double> real_distribution;     // [0, 1)
    explicit RefRandom(long long seed) { generator.seed(seed); }
    double rand_real() { return real_distribution(generator); }
    int rand_int(int max_val = std::numeric_limits<int>::max()) { return (int)(rand_real() * max_val); }
};

// glibc's rand() (random_r.c, TYPE_3: the additive feedback generator x^31 + x^3 + 1 over 31-bit outputs,
// state filled from the seed by the Lehmer generator 16807 mod 2^31 - 1, first 310 outputs discarded).
// tests/test_abi_cpu.py checks it against the C library's own rand().
struct GlibcRand {
    int32_t r[34];
    int f = 3, b = 0;           // front / rear indices into r[3..33]
    explicit GlibcRand(unsigned seed = 1) {
        int32_t *state = r + 3;     // 31 words (r[0..2] unused; keeps the textbook indices readable)
        if (seed == 0) seed = 1;
        state[0] = (int32_t)seed;
        for (int i = 1; i < 31; i++) {
            const long hi = state[i - 1] / 127773, lo = state[i - 1] % 127773;
            long word = 16807 * lo - 2836 * hi;
            if (word < 0) word += 2147483647;
            state[i] = (int32_t)word;
        }
        f = 3;
        b = 0;
        for (int i = 0; i < 310; i++) (void)next();
    }
    int next() {
        int32_t *state = r + 3;
        const uint32_t val = (uint32_t)state[f] + (uint32_t)state[b];
        state[f] = (int32_t)val;
        const int result = (int)(val >> 1);
        if (++f >= 31) f = 0;
        if (++b >= 31) b = 0;
        return result;
    }
};

// The stream the reference draws from -- the restated libc one (library-wide, as the reference's is process-wide) --
// or, when the caller seeds, a generator of the caller's own.  (Inline: an oversampling round draws once per point.)
int reference_rand_next();          // one draw from the library-wide generator, under its lock
struct RandStream {
    bool shared;
    GlibcRand own;
    explicit RandStream(long seed) : shared(seed < 0), own(seed < 0 ? 1u : (unsigned)seed + 1u) {}
    int operator()() { return shared ? reference_rand_next() : own.next(); }
};

// The reference library's other draws from rand(), made by the legacy entry points so that the library's stream
// stays in step with the reference's: one per Gaussian that GMM::load constructs (gmm.cc:671-676), one for the
// trainer plus one per Gaussian in train_model_from_ubm (gmmubm.cc:29-38).
void burn_reference_rand(int count);
// fork support (common.cpp, fork_proxy.cpp): a forked child gets a fresh lock; the generator's state travels to the helper
// process that computes on a forked child's behalf and back, so that the library-wide stream stays the one the reference's
// process-wide rand() would be
void reference_rand_fork_child();
void reference_rand_state(int32_t *words36, bool set);
// the first `count` values of a fresh generator (test hook: compared with the C library's rand())
void reference_rand_sample(int *out, int count);

}  // namespace sr
