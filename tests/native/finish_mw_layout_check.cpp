// finish_mw_layout_check.cpp - the layout rule and the option parser of the microwave finish kernel (finish_mw_layout.hpp) without a GPU.
// stdin, one request per line:
//   rule <nprof> <nlay_max> <nwn> <cus> <nA> <NPTABS> <sliced> <opt>   -> "waves=<NW or 0> lds=<bytes of a column workgroup of 4 waves>"
//   parse [<value>]                                                    -> "ok=<0|1> opt=<FINISH_MW_*>"
// (tests/test_finish_mw_column_cpu.py)
#include <cstdio>
#include <cstring>

#include "../../monortm_amd/csrc/finish_mw_layout.hpp"

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        line[strcspn(line, "\n")] = 0;
        if (!strncmp(line, "rule ", 5)) {
            monortm_dev::MwLayoutIn in{};
            int sliced = 0;
            if (sscanf(line + 5, "%d %d %d %d %d %d %d %d", &in.nprof, &in.nlay_max, &in.nwn, &in.cus, &in.nA, &in.NPTABS, &sliced, &in.opt) != 8) return 2;
            in.sliced = sliced != 0;
            printf("waves=%d lds=%zu\n", monortm_dev::finish_mw_col_waves(in), monortm_dev::finish_mw_col_lds(in.nA, in.NPTABS, 4));
        } else if (!strncmp(line, "parse", 5)) {
            int opt = -1;
            const bool ok = monortm_dev::finish_mw_parse(line[5] ? line + 6 : "", &opt);
            printf("ok=%d opt=%d\n", ok ? 1 : 0, ok ? opt : -1);
        } else return 2;
    }
    return 0;
}
