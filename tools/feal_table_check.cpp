// feal_table_check.cpp — prints the host tables of csrc/resp_tables.h (what gw_create uploads) as
// C99 hex floats, one per line: "resp vm va value" then "feal vm va value".  A stand-alone host
// program (no HIP): tests/test_feal_cpu.py compares the lines with numpy's own evaluation.
//   c++ -std=c++17 -Imarl-responsible-nav_amd/csrc tools/feal_table_check.cpp -o feal_table_check
#include <cstdio>

#include "resp_tables.h"

int main() {
    double t[200];
    gwtab::fill(t);
    for (int k = 0; k < 2; ++k)
        for (int vm = 0; vm < 10; ++vm)
            for (int va = 0; va < 10; ++va)
                std::printf("%s %d %d %a\n", k ? "feal" : "resp", vm, va, t[100 * k + 10 * vm + va]);
    return 0;
}
