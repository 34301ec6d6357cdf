// resp_map_check.cpp -- stand-alone host program around the bin rule of gw_resp_map_accum (csrc/resp_map.h),
// for tests/test_resp_map_cpu.py, which builds it with AddressSanitizer + UBSan and compares its answers with a
// numpy restatement of the rule.
//
// stdin, one sample per line:   set_act  cell_i  cell_j  HW      (integers in any strtol form)
// stdout, binary: per sample, for every set_mdr = 0 .. 0xFFFF in order, the two int64 indices
//     caused received     of resp_map::bins(set_mdr | set_act << 16, cell_i, cell_j, HW).
// Each index also increments a heap array of exactly 2 * HW * 100 counters, as the kernel does: an index
// outside the buffer is an AddressSanitizer error.  The sum of the counters must be 2 * 65536.
//
//     c++ -std=c++17 -I marl-responsible-nav_amd/csrc tools/resp_map_check.cpp -o resp_map_check
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "resp_map.h"

int main() {
    std::string line;
    long n = 0;
    std::vector<int64_t> out(2 * 65536);
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::vector<std::string> tok;
        for (std::string w; in >> w;) tok.push_back(w);
        if (tok.size() != 4) {
            std::fprintf(stderr, "sample %ld: %zu fields, expected 4\n", n, tok.size());
            return 2;
        }
        const uint32_t set_act = (uint32_t)std::strtoul(tok[0].c_str(), nullptr, 0) & 0xFFFFu;
        const int32_t cell_i = (int32_t)std::strtol(tok[1].c_str(), nullptr, 0);
        const int32_t cell_j = (int32_t)std::strtol(tok[2].c_str(), nullptr, 0);
        const int32_t HW = (int32_t)std::strtol(tok[3].c_str(), nullptr, 0);
        if (HW < 1 || HW > 1 << 20) {
            std::fprintf(stderr, "sample %ld: HW out of range\n", n);
            return 2;
        }
        std::vector<uint64_t> counts((size_t)2 * HW * resp_map::NV * resp_map::NV);
        for (uint32_t set_mdr = 0; set_mdr <= 0xFFFFu; ++set_mdr) {
            const resp_map::Bins b = resp_map::bins(set_mdr | (set_act << 16), cell_i, cell_j, HW);
            counts.data()[b.caused] += 1;  // raw pointer: the sanitizer's check, not the vector's
            counts.data()[b.received] += 1;
            out[2 * set_mdr] = b.caused;
            out[2 * set_mdr + 1] = b.received;
        }
        uint64_t total = 0;
        for (uint64_t c : counts) total += c;
        if (total != 2u * 65536u) {
            std::fprintf(stderr, "sample %ld: %llu increments\n", n, (unsigned long long)total);
            return 3;
        }
        if (std::fwrite(out.data(), sizeof(int64_t), out.size(), stdout) != out.size()) return 4;
        ++n;
    }
    std::fprintf(stderr, "%ld samples\n", n);
    return 0;
}
