// ref_rand.cpp -- the library-wide restated rand() and what keeps it in step with the reference's (ref_rand.hpp).
#include "ref_rand.hpp"

#include <mutex>
#include <new>

namespace sr {

namespace {
std::mutex g_rand_mutex;
GlibcRand g_reference_rand;       // what rand() would return in a process where the reference library is its only user
}  // namespace

int reference_rand_next() {
    std::lock_guard<std::mutex> lock(g_rand_mutex);
    return g_reference_rand.next();
}

void burn_reference_rand(int count) {
    std::lock_guard<std::mutex> lock(g_rand_mutex);
    for (int i = 0; i < count; i++) (void)g_reference_rand.next();
}
void reference_rand_fork_child() { new (&g_rand_mutex) std::mutex(); }
void reference_rand_state(int32_t *words36, bool set) {
    std::lock_guard<std::mutex> lock(g_rand_mutex);
    if (set) {
        for (int i = 0; i < 34; i++) g_reference_rand.r[i] = words36[i];
        g_reference_rand.f = words36[34];
        g_reference_rand.b = words36[35];
    } else {
        for (int i = 0; i < 34; i++) words36[i] = g_reference_rand.r[i];
        words36[34] = g_reference_rand.f;
        words36[35] = g_reference_rand.b;
    }
}
void reference_rand_sample(int *out, int count) {
    GlibcRand g;
    for (int i = 0; i < count; i++) out[i] = g.next();
}

}  // namespace sr
