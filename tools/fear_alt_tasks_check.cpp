// Stand-alone CPU check of fear_alt_kernel's task-list arithmetic (csrc/fear_alt_tasks.h): build it
// with a host compiler and the sanitizers and run it,
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I marl-responsible-nav_amd/csrc tools/fear_alt_tasks_check.cpp -o /tmp/fear_alt_tasks_check
// It walks every (N, K, close count, task) the kernel can meet, the actor search of a run over a subset
// of the actors (actor_of, csrc/fear_alt_core.h's callers), and the out-of-range inputs the
// kernel clamps, and indexes real arrays of the kernel's LDS sizes so that a bad index is a
// sanitizer error, not a silent pass.  tests/test_fear_alt_cpu.py runs it when a compiler is there.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fear_alt_tasks.h"

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

// actor_of against the straightforward walk: the actors of `sel` in ascending order, each with its tasks in order.
// Actors outside sel keep their counts (the kernels' plan holds every actor's), actors from K on have none.
template <int N>
long check_actor_of(uint32_t sel, const int (&tcount)[N]) {
    using namespace fear_alt;
    int ti = 0;
    for (int k = 0; k < N; ++k) {
        if (!((sel >> k) & 1u)) continue;
        for (int r = 0; r < tcount[k]; ++r, ++ti) {
            const Actor t = actor_of<N>(sel, tcount, ti);
            CHECK(t.k == k && t.r == r);
        }
    }
    // past the total: an actor inside the array, a task number decode clamps
    const Actor past = actor_of<N>(sel, tcount, ti);
    CHECK(past.k >= 0 && past.k < N && past.r >= 0);
    return ti;
}

// Every K <= N and non-zero sel below 1 << K.  Close counts: every combination over the selected actors where
// that is at most N^FULL vectors (all of them for N <= 4); beyond, the search being one comparison and one
// subtraction per actor position, every count 1..N at every selected position over a mixed background, and
// every count at all positions at once.  Every ti below the total each time.
template <int N>
long check_actor_of_all() {
    using namespace fear_alt;
    constexpr int FULL = N <= 4 ? N : 3;
    long walked = 0;
    for (int K = 1; K <= N; ++K) {
        for (uint32_t sel = 1; sel < (1u << K); ++sel) {
            int tcount[N];
            auto fill = [&](auto count_of) {  // count_of(q): close count of actor q < K
                for (int q = 0; q < N; ++q) tcount[q] = q < K ? per_actor(count_of(q)) : 0;
                walked += check_actor_of<N>(sel, tcount);
            };
            const int m = __builtin_popcount(sel);
            if (m <= FULL) {
                int vectors = 1;
                for (int i = 0; i < m; ++i) vectors *= N;
                for (int v = 0; v < vectors; ++v)
                    fill([&](int q) {
                        if (!((sel >> q) & 1u)) return 1 + (q + v) % N;  // not selected: must not matter
                        int digit = v;
                        for (int i = __builtin_popcount(sel & ((1u << q) - 1u)); i > 0; --i) digit /= N;
                        return 1 + digit % N;
                    });
            } else {
                for (int c = 1; c <= N; ++c) {
                    fill([&](int) { return c; });
                    for (int at = 0; at < K; ++at)
                        if ((sel >> at) & 1u) fill([&](int q) { return q == at ? c : 1 + (q * 5 + 3) % N; });
                }
            }
        }
    }
    return walked;
}

int main() {
    using namespace fear_alt;
    static_assert(max_per_env(4, 2) == 450, "N = 4, K = 2");
    static_assert(max_per_env(8, 2) == 1026, "N = 8, K = 2");
    static_assert(max_per_env(8, 8) == 4104, "N = 8, K = 8");
    static_assert(bit_words(8, 8) == 576, "valid-bit words per env");
    long tasks = 0;
    for (int N = 1; N <= 8; ++N) {
        for (int K = 1; K <= N; ++K) {
            std::vector<uint32_t> vb((size_t)bit_words(N, K), 0u);  // the kernel's [K][9][N] words of one env
            CHECK(bit_words(N, K) <= bit_words(N, N) && bit_words(N, N) <= 576);
            for (int k = 0; k < K; ++k) {
                for (uint32_t others = 0; others < (1u << N); ++others) {
                    if ((others >> k) & 1u) continue;  // the close set without the actor
                    const uint32_t cl = others | (1u << k);
                    const int c = __builtin_popcount(cl);
                    CHECK(c >= 1 && c <= N);
                    const int T = per_actor(c);
                    CHECK(T == 9 * (1 + 8 * (c - 1)) && T <= max_per_env(N, 1));
                    std::vector<uint8_t> seen((size_t)T, 0);
                    for (int r = 0; r < T; ++r) {
                        const Task t = decode(r, c);
                        CHECK(t.a >= 0 && t.a < NA);
                        CHECK(t.slot >= -1 && t.slot <= c - 2);
                        CHECK(t.bi >= 0 && t.bi < 8);
                        CHECK(encode(t.a, t.slot, t.bi, c) == r);
                        seen[(size_t)r] += 1;
                        int j = -1;
                        if (t.slot >= 0) {
                            j = nth_agent(others, t.slot);
                            CHECK(j >= 0 && j < N && j != k && ((others >> j) & 1u));
                            // the slot-th set bit: exactly `slot` set bits below it
                            CHECK(__builtin_popcount(others & ((1u << j) - 1u)) == t.slot);
                            for (int own = 0; own < NA; ++own) {
                                const int b = alternative(t.bi, own);
                                CHECK(b >= 0 && b < NA && b != own);
                                vb[(size_t)((k * NA + t.a) * N + j)] |= 1u << b;
                            }
                        } else {
                            for (int n = 0; n < N; ++n) vb[(size_t)((k * NA + t.a) * N + n)] |= 0x1FFu;
                        }
                        ++tasks;
                    }
                    for (int r = 0; r < T; ++r) CHECK(seen[(size_t)r] == 1);
                    CHECK(nth_agent(others, c - 1) == -1);  // one past the last close agent
                    // out-of-range task numbers clamp to the last task
                    const Task lo = decode(-5, c), hi = decode(T + 1000, c);
                    CHECK(encode(lo.a, lo.slot, lo.bi, c) == 0);
                    CHECK(encode(hi.a, hi.slot, hi.bi, c) == T - 1);
                }
            }
            for (uint32_t w : vb) CHECK(w <= 0x1FFu);
        }
    }
    // the 8 alternatives of an agent are its 8 other actions, ascending
    for (int own = 0; own < NA; ++own) {
        uint32_t m = 0;
        int prev = -1;
        for (int bi = 0; bi < 8; ++bi) {
            const int b = alternative(bi, own);
            CHECK(b > prev);
            prev = b;
            m |= 1u << b;
        }
        CHECK(m == (0x1FFu & ~(1u << own)));
    }
    const long searched = check_actor_of_all<2>() + check_actor_of_all<3>() + check_actor_of_all<4>() +
                          check_actor_of_all<5>() + check_actor_of_all<6>() + check_actor_of_all<7>() +
                          check_actor_of_all<8>();
    std::printf("fear_alt task arithmetic ok: %ld tasks walked, %ld actor searches\n", tasks, searched);
    return 0;
}
