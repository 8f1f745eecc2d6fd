// trig_host_check.hip — glibc_sincosf_both (s2m_glibc_trig.hpp) against the build host's sinf / cosf, bit for bit, on the CPU.
//
//   hipcc --offload-arch=gfx950 --cuda-host-only -O2 -ffp-contract=off -o trig_host_check tools/micro/trig_host_check.hip -lm
//   ./trig_host_check            prints one line per mismatching argument: "<argument bits, hex> <s|c|sc>", then a summary line
//
// Arguments: 2e6 random values in [-4, 4]; both neighbours (up to three ulps each side, both signs) of the three branch
// boundaries 2^-12, 0x1.921FB6p-1 (pi/4) and 120; k*pi/2 and its neighbours up to two ulps each side for k = -76..76.
// tests/test_trig_host_cpu.py builds and runs it and holds the admitted mismatch set.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../liorf_amd/csrc/s2m_glibc_trig.hpp"

static uint32_t bits_of(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float step_ulps(float x, int n)
{
    for (int i = 0; i < (n < 0 ? -n : n); i++) x = nextafterf(x, n < 0 ? -INFINITY : INFINITY);
    return x;
}

int main()
{
    std::vector<float> xs;
    uint64_t s = 0x9E3779B97F4A7C15ull;                       // splitmix64: the same arguments on every run
    for (int i = 0; i < 2000000; i++) {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        xs.push_back((float)((double)(z >> 11) * (8.0 / 9007199254740992.0) - 4.0));
    }
    const float edges[3] = { 0x1p-12f, 0x1.921FB6p-1f, 120.0f };
    for (float e : edges)
        for (int d = -3; d <= 3; d++) { const float v = step_ulps(e, d); xs.push_back(v); xs.push_back(-v); }
    for (int k = -76; k <= 76; k++)
        for (int d = -2; d <= 2; d++) xs.push_back(step_ulps((float)((double)k * 0x1.921FB54442D18p0), d));

    volatile float vx;                                        // the library calls see a run-time argument
    size_t bad = 0;
    for (float x : xs) {
        float sn, cs;
        s2m::glibc_sincosf_both(x, sn, cs);
        vx = x;
        const float rs = sinf(vx), rc = cosf(vx);
        const bool ms = bits_of(sn) != bits_of(rs), mc = bits_of(cs) != bits_of(rc);
        if (ms || mc) { printf("%08x %s\n", bits_of(x), ms && mc ? "sc" : (ms ? "s" : "c")); bad++; }
    }
    printf("checked %zu mismatches %zu\n", xs.size(), bad);
    return 0;
}
