// crash_shield_check.cpp -- stand-alone host program around the visit rule of gw_crash_shield_joint
// (csrc/crash_shield.h: the safe mask of csrc/step_preview.h, the pick of csrc/fear_shield.h, the unavoidable
// bit), for tests/test_crash_shield_joint_cpu.py, which builds it with AddressSanitizer + UBSan and compares its
// answers with the rule as include/gridenv.h states it.
//
// stdin, one visit per line (integers in any strtoul form, hex included; floats in any strtod / strtof form):
//     has_mask  mask  crash9  cur  use_fear  tau  has_probs  t[0..8]  pr[0..8]
// stdout, one line per visit:  action flags      (flags: bit 0 replaced, bit 1 stuck, bit 5 unavoidable)
//
//     c++ -std=c++17 -I marl-responsible-nav_amd/csrc tools/crash_shield_check.cpp -o crash_shield_check
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "crash_shield.h"

int main() {
    std::string line;
    long n = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::vector<std::string> tok;
        for (std::string w; in >> w;) tok.push_back(w);
        const size_t need = 7 + 2 * fear_shield::NA;
        if (tok.size() != need) {
            std::fprintf(stderr, "visit %ld: %zu fields, expected %zu\n", n, tok.size(), need);
            return 2;
        }
        const bool has_mask = std::atoi(tok[0].c_str()) != 0;
        const uint32_t mask = (uint32_t)std::strtoul(tok[1].c_str(), nullptr, 0);
        const uint32_t crash9 = (uint32_t)std::strtoul(tok[2].c_str(), nullptr, 0);
        const int cur = std::atoi(tok[3].c_str());
        const bool use_fear = std::atoi(tok[4].c_str()) != 0;
        const double tau = std::strtod(tok[5].c_str(), nullptr);
        const bool has_probs = std::atoi(tok[6].c_str()) != 0;
        // exactly nine entries each, on the heap: a read past a row is an AddressSanitizer error
        std::vector<double> t(fear_shield::NA);
        std::vector<float> pr(fear_shield::NA);
        for (int a = 0; a < fear_shield::NA; ++a) {
            t[a] = std::strtod(tok[7 + a].c_str(), nullptr);
            pr[a] = std::strtof(tok[7 + fear_shield::NA + a].c_str(), nullptr);
        }
        // without FeAR the rule reads no table at all: hand it none
        const crash_shield::Visit v = crash_shield::visit(use_fear ? t.data() : nullptr, cur, has_mask, mask, crash9,
                                                          has_probs ? pr.data() : nullptr, use_fear, tau);
        std::printf("%d %d\n", v.action, v.flags);
        ++n;
    }
    std::fprintf(stderr, "%ld visits\n", n);
    return 0;
}
