// The slot words of lines_ms_kernel's reach rule (monortm_amd/csrc/ms_reach.hpp) from the command line: one case per line of stdin, its
// 16-bit word on one line of stdout.  Built with the host compiler and driven by tests/test_ms_reach_cpu.py (no GPU: host code only).
// Input, separated by blanks (doubles in any form strtod reads: hexadecimal, nan, inf):
//   nwn LPS every x max_abs_shift wn[0] .. wn[nwn - 1]
// The margin is ms_reach_pad(max_abs_shift), as ms_reach_kernel forms it.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../monortm_amd/csrc/ms_reach.hpp"

using namespace monortm_dev;

int main() {
    static char line[4096];
    double wn[64];
    while (std::fgets(line, sizeof line, stdin)) {
        if (line[0] == '\n' || line[0] == '#') continue;
        char *p = line, *q;
        const long nwn = std::strtol(p, &q, 10); p = q;
        const long LPS = std::strtol(p, &q, 10); p = q;
        const long every = std::strtol(p, &q, 10); p = q;
        if (nwn < 0 || nwn > 64 || LPS < 1) { std::fprintf(stderr, "ms_reach_check: nwn = %ld, LPS = %ld in: %s", nwn, LPS, line); return 2; }
        const double x = std::strtod(p, &q);
        if (q == p) { std::fprintf(stderr, "ms_reach_check: no centre in: %s", line); return 2; }
        p = q;
        const double mas = std::strtod(p, &q);
        if (q == p) { std::fprintf(stderr, "ms_reach_check: no shift bound in: %s", line); return 2; }
        p = q;
        for (long i = 0; i < nwn; i++) {
            wn[i] = std::strtod(p, &q);
            if (q == p) { std::fprintf(stderr, "ms_reach_check: %ld of %ld channels in: %s", i, nwn, line); return 2; }
            p = q;
        }
        std::printf("%u\n", ms_reach_word(wn, (int)nwn, (int)LPS, x, every != 0, ms_reach_pad(mas)));
    }
    return 0;
}
