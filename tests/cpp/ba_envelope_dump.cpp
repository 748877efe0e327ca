// ba_envelope_dump.cpp -- runs mvs_bas::check_csr and mvs_bas::plan of mvslam_amd/csrc/ba_envelope.hpp (the host planning of the
// sparse bundle adjustment) on a problem read from a text file (F P O, obs_off, obs_frame) and prints
// every list of the plan, one per line, for tests/test_ba_sparse_host.py to compare with a brute-force restatement.  Built with
// the host sanitizers and run as a program of its own.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ba_envelope.hpp"

static void line(const char *name, const std::vector<int32_t> &v)
{
    std::printf("%s", name);
    for (int32_t x : v)
        std::printf(" %d", x);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 2)
        return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f)
        return 2;
    int F = 0, P = 0, O = 0;
    if (std::fscanf(f, "%d %d %d", &F, &P, &O) != 3 || F < 1 || P < 1 || O < 0)
        return 2;
    std::vector<int32_t> off((size_t)P + 1), fr((size_t)O);
    for (auto &x : off)
        if (std::fscanf(f, "%d", &x) != 1)
            return 2;
    for (auto &x : fr)
        if (std::fscanf(f, "%d", &x) != 1)
            return 2;
    std::fclose(f);
    const int bad = mvs_bas::check_csr(F, P, O, off.data(), fr.data());
    std::printf("check %d\n", bad);
    if (bad)
        return 0;
    const mvs_bas::Plan p = mvs_bas::plan(F, P, O, off.data(), fr.data());
    std::printf("blocks %lld\npairs %lld\nwidest %d\nfits %d\n", (long long)p.blocks, (long long)p.pairs, p.widest, (int)p.fits());
    line("first", p.first);
    line("row_off", p.row_off);
    line("blk_row", p.blk_row);
    line("last", p.last);
    line("obs_point", p.obs_point);
    line("fr_off", p.fr_off);
    line("fr_obs", p.fr_obs);
    line("pair_off", p.pair_off);
    line("pair_a", p.pair_a);
    line("pair_c", p.pair_c);
    return 0;
}
