// step_preview_check.cpp -- stand-alone host program around the safe-mask rule of gw_step_preview
// (csrc/step_preview.h) and the pick the crash-aware shield makes from it (csrc/fear_shield.h on a zero table
// with tau = 0, the safe mask in the action mask's place), for tests/test_step_preview_rule.py, which builds it
// with AddressSanitizer + UBSan and compares its answers with the rule as include/gridenv.h states it.
//
// stdin, one case per line (integers in any strtoul form, hex included; floats in any strtof form):
//     has_mask  mask  crash9  p  pr[0..8]
// stdout, one line per case:  safe_mask action flags
//
//     c++ -std=c++17 -I marl-responsible-nav_amd/csrc tools/step_preview_check.cpp -o step_preview_check
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fear_shield.h"
#include "step_preview.h"

int main() {
    std::string line;
    long n = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::vector<std::string> tok;
        for (std::string w; in >> w;) tok.push_back(w);
        const size_t need = 4 + fear_shield::NA;
        if (tok.size() != need) {
            std::fprintf(stderr, "case %ld: %zu fields, expected %zu\n", n, tok.size(), need);
            return 2;
        }
        const bool has_mask = std::atoi(tok[0].c_str()) != 0;
        const uint32_t mask = (uint32_t)std::strtoul(tok[1].c_str(), nullptr, 0);
        const uint32_t crash9 = (uint32_t)std::strtoul(tok[2].c_str(), nullptr, 0);
        const int p = std::atoi(tok[3].c_str());
        // exactly nine entries each, on the heap: a read past a row is an AddressSanitizer error
        std::vector<double> zero(fear_shield::NA, 0.0);
        std::vector<float> pr(fear_shield::NA);
        for (int a = 0; a < fear_shield::NA; ++a) pr[a] = std::strtof(tok[4 + a].c_str(), nullptr);
        const uint32_t safe = step_preview::safe_mask(has_mask, mask, crash9);
        const fear_shield::Pick r = fear_shield::pick(zero.data(), p, safe, pr.data(), 0.0, true);
        std::printf("%u %d %d\n", safe, r.action, r.flags);
        ++n;
    }
    std::fprintf(stderr, "%ld cases\n", n);
    return 0;
}
