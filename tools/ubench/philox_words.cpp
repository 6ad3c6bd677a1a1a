// The words of the project's own Philox (csrc/emx_rng.hpp) for counters and keys read from standard input: one line of six hex
// words "c0 c1 c2 c3 k0 k1" in, one line of eight hex words out -- philox4x32<7> then philox4x32<10>.
// Built and run by tests/test_gauss_noise_ref_cpu.py, which compares them with the NumPy reference of tests/gauss_noise_ref.py.
#include <cstdio>
#include "emx_rng.hpp"
using namespace emx;
int main() {
    unsigned c0, c1, c2, c3, k0, k1;
    while (std::scanf("%x %x %x %x %x %x", &c0, &c1, &c2, &c3, &k0, &k1) == 6) {
        const Philox4 a = philox4x32<7>(c0, c1, c2, c3, k0, k1), b = philox4x32<10>(c0, c1, c2, c3, k0, k1);
        std::printf("%08x %08x %08x %08x %08x %08x %08x %08x\n", a.v[0], a.v[1], a.v[2], a.v[3], b.v[0], b.v[1], b.v[2], b.v[3]);
    }
    return 0;
}
