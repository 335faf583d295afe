// TEST INFRASTRUCTURE: walks csrc/comb_quotient.h on the host (tests/test_offspring_fill_cpu.py).
//   comb_quotient_driver IN OUT: IN holds triples of little-endian uint64 {hi, lo, d}, OUT receives one uint64 quotient each.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "comb_quotient.h"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    std::vector<uint64_t> q;
    uint64_t t[3];
    while (fread(t, sizeof(uint64_t), 3, in) == 3) q.push_back(slam::quotient_below_2_32(t[0], t[1], t[2]));
    fclose(in);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 4;
    const size_t done = fwrite(q.data(), sizeof(uint64_t), q.size(), out);
    return fclose(out) == 0 && done == q.size() ? 0 : 5;
}
