// fear_shield_check.cpp -- stand-alone host program around the shield's selection rule (csrc/fear_shield.h),
// for tests/test_fear_preview_cpu.py, which builds it with AddressSanitizer + UBSan and compares its answers
// with a numpy restatement of the rule.
//
// stdin, one case per line (floats in any strtod form, hex included):
//     p  mask  shielded  tau  has_probs  t[0..8]  [pr[0..8] if has_probs]
// stdout, one line per case:  action flags
//
//     c++ -std=c++17 -I marl-responsible-nav_amd/csrc tools/fear_shield_check.cpp -o fear_shield_check
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "fear_shield.h"

int main() {
    std::string line;
    long n = 0;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::vector<std::string> tok;
        for (std::string w; in >> w;) tok.push_back(w);
        if (tok.size() < 5) {
            std::fprintf(stderr, "case %ld: too few fields\n", n);
            return 2;
        }
        const int p = std::atoi(tok[0].c_str());
        const uint32_t mask = (uint32_t)std::strtoul(tok[1].c_str(), nullptr, 0);
        const bool shielded = std::atoi(tok[2].c_str()) != 0;
        const double tau = std::strtod(tok[3].c_str(), nullptr);
        const bool has_probs = std::atoi(tok[4].c_str()) != 0;
        const size_t need = 5 + fear_shield::NA * (has_probs ? 2 : 1);
        if (tok.size() != need) {
            std::fprintf(stderr, "case %ld: %zu fields, expected %zu\n", n, tok.size(), need);
            return 2;
        }
        // exactly nine entries each, on the heap: a read past a row is an AddressSanitizer error
        std::vector<double> t(fear_shield::NA);
        std::vector<float> pr(has_probs ? fear_shield::NA : 0);
        for (int a = 0; a < fear_shield::NA; ++a) t[a] = std::strtod(tok[5 + a].c_str(), nullptr);
        for (int a = 0; has_probs && a < fear_shield::NA; ++a)
            pr[a] = std::strtof(tok[5 + fear_shield::NA + a].c_str(), nullptr);
        const fear_shield::Pick r = fear_shield::pick(t.data(), p, mask, has_probs ? pr.data() : nullptr, tau, shielded);
        std::printf("%d %d\n", r.action, r.flags);
        ++n;
    }
    std::fprintf(stderr, "%ld cases\n", n);
    return 0;
}
