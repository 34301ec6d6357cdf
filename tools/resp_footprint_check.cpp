// resp_footprint_check.cpp -- stand-alone host program around the bin rule of gw_resp_footprint_accum
// (csrc/resp_footprint.h), for tests/test_resp_footprint_cpu.py, which builds it with AddressSanitizer + UBSan.
//
// No arguments: the sweep.  For every R in 1..15, a set of map shapes (H, W), cells including -1 and HW,
// actions including -1, 9 and INT_MAX, and a set of words that reaches every (vm, va), the header's bin is
// compared with a plain restatement written here from the op's contract, and each bin increments a heap array
// of exactly 2 * 9 * O * 100 counters in both planes, as the kernel does: an index outside the buffer is an
// AddressSanitizer error.  Prints the number of bins checked; a mismatch or a lost increment is exit status 3.
//
// "-" as the only argument: stdin, one sample per line:   word  cell_i  cell_j  a_i  W  HW  R   (any strtol
// form); stdout: one bin per line, for a comparison with another restatement.
//
//     c++ -std=c++17 -I marl-responsible-nav_amd/csrc tools/resp_footprint_check.cpp -o resp_footprint_check
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "resp_footprint.h"

namespace {

// the contract restated: bit loops, long long arithmetic, no helper of the header
long long plain_bin(unsigned long word, long long ci, long long cj, long long a, long long W, long long HW, long long R) {
    int vm = 0, va = 0;
    for (int b = 0; b < 9; ++b) {
        vm += (word >> b) & 1;
        va += (word >> (16 + b)) & 1;
    }
    if (ci < 0) ci = 0;
    if (ci > HW - 1) ci = HW - 1;
    if (cj < 0) cj = 0;
    if (cj > HW - 1) cj = HW - 1;
    if (a < 0 || a > 8) a = 0;
    const long long dr = cj / W - ci / W, dc = cj % W - ci % W, S = 2 * R + 1, O = S * S + 1;
    long long o = S * S;
    if (dr >= -R && dr <= R && dc >= -R && dc <= R) o = (dr + R) * S + (dc + R);
    return ((a * O + o) * 10 + vm) * 10 + va;
}

int from_stdin() {
    std::string line;
    long n = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::vector<long long> v;
        for (std::string w; in >> w;) v.push_back(std::strtoll(w.c_str(), nullptr, 0));
        if (v.size() != 7 || v[4] < 1 || v[5] < 1 || v[6] < 0 || v[6] > 15) {
            std::fprintf(stderr, "sample %ld: expected word cell_i cell_j a_i W HW R\n", n);
            return 2;
        }
        std::printf("%lld\n", (long long)resp_footprint::bin((uint32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3],
                                                             (int32_t)v[4], (int32_t)v[5], (int32_t)v[6]));
        ++n;
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && std::string(argv[1]) == "-") return from_stdin();
    // words: every (vm, va) through low-bit runs, plus bits outside the nine that must be ignored
    std::vector<uint32_t> words;
    for (int vm = 0; vm <= 9; ++vm)
        for (int va = 0; va <= 9; ++va) words.push_back(((1u << vm) - 1u) | (((1u << va) - 1u) << 16));
    for (uint32_t w : {0xFFFFFFFFu, 0xFE00FE00u, 0x01550155u, 0x8001AAAAu, 0x02000100u}) words.push_back(w);
    const int32_t shapes[][2] = {{1, 1}, {1, 8}, {13, 3}, {2, 2}, {7, 9}, {32, 32}, {64, 64}, {3, 40}};
    const int32_t acts[] = {-1, 0, 1, 4, 8, 9, INT_MAX, INT_MIN};
    long long checked = 0;
    for (int32_t R = 1; R <= 15; ++R) {
        const long long O = resp_footprint::offsets(R), plane = 9 * O * 100;
        if (O != (2LL * R + 1) * (2 * R + 1) + 1) return 3;
        std::vector<uint64_t> counts((size_t)(2 * plane));
        long long added = 0;
        for (const auto &hw : shapes) {
            const int32_t H = hw[0], W = hw[1], HW = H * W;
            // cells: the corners, the out-of-range ones, and a stride through the map
            std::vector<int32_t> cells = {-1, 0, HW - 1, HW, INT_MAX, INT_MIN, W - 1, HW - W};
            for (int32_t c = 0; c < HW; c += (HW > 24 ? HW / 19 + 1 : 1)) cells.push_back(c);
            for (int32_t ci : cells)
                for (int32_t cj : cells)
                    for (int32_t a : acts)
                        for (size_t w = (size_t)((ci ^ cj ^ a) & 7); w < words.size(); w += 8) {  // a rotating eighth
                            const int64_t b = resp_footprint::bin(words[w], ci, cj, a, W, HW, R);
                            const long long want = plain_bin(words[w], ci, cj, a, W, HW, R);
                            if (b != want || b < 0 || b >= plane) {
                                std::fprintf(stderr, "R %d W %d HW %d cells %d %d a %d word %#x: bin %lld, expected %lld\n",
                                             R, W, HW, ci, cj, a, words[w], (long long)b, want);
                                return 3;
                            }
                            counts.data()[b] += 1;  // raw pointer: the sanitizer's check, not the vector's
                            counts.data()[plane + b] += 1;
                            added += 2;
                            ++checked;
                        }
        }
        uint64_t total = 0;
        for (uint64_t c : counts) total += c;
        if (total != (uint64_t)added) {
            std::fprintf(stderr, "R %d: %llu of %lld increments\n", R, (unsigned long long)total, added);
            return 3;
        }
    }
    std::printf("%lld bins checked\n", checked);
    return 0;
}
