// The routing function of the dense dispatcher (s2d_amd/csrc/gemm_route.h) as a stand-alone host program: no HIP, no GPU.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Is2d_amd/csrc scripts/gemm_route_main.cpp -o gemm_route_main
//   ./gemm_route_main grid [setting]    the grid of scripts/gemm_route_grid.h under switch setting `setting` (default: every setting):
//                                       launches per route name
//   ./gemm_route_main lines             stdin: one launch per line, GEMM_D_COUNT integers, the flag bits, 13 switch values ('u': the default);
//                                       stdout: its route name
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>

#include "gemm_route_grid.h"

int main(int argc, char **argv)
{
    char name[128];
    int sw[GEMM_SWITCH_COUNT];
    if (argc >= 2 && !strcmp(argv[1], "grid")) {
        const int first = argc >= 3 ? atoi(argv[2]) : 0, last = argc >= 3 ? first + 1 : GEMM_SWITCH_SETTING_COUNT;
        if (first < 0 || last > GEMM_SWITCH_SETTING_COUNT) return 2;
        for (int i = first; i < last; ++i) {
            gemm_switch_setting(i, sw);
            std::map<std::string, long> hist;
            const long n = gemm_route_grid([&](const long *v, int flags) {
                if (s2d_gemm_route_text(v, flags, sw, name, sizeof name) < 0) abort();
                ++hist[name];
            });
            printf("setting %d (switch %d = %d): %ld launches\n", i, GEMM_SWITCH_SETTINGS[i].index, GEMM_SWITCH_SETTINGS[i].value, n);
            for (const auto &h : hist) printf("  %-60s %ld\n", h.first.c_str(), h.second);
        }
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "lines")) {
        char line[1024];
        while (fgets(line, sizeof line, stdin)) {
            long v[GEMM_D_COUNT];
            char *s = line;
            for (int i = 0; i < GEMM_D_COUNT; ++i) v[i] = strtol(s, &s, 10);
            const int flags = (int)strtol(s, &s, 10);
            gemm_switch_setting(0, sw);
            for (int i = 0; i < GEMM_SWITCH_COUNT; ++i) {
                while (*s == ' ') ++s;
                if (*s == 'u') ++s;
                else sw[i] = (int)strtol(s, &s, 10);
            }
            if (s2d_gemm_route_text(v, flags, sw, name, sizeof name) < 0) return 1;
            puts(name);
        }
        return 0;
    }
    fprintf(stderr, "usage: %s grid [setting] | lines\n", argv[0]);
    return 2;
}
