// icp_close_main.cpp — liorf_amd/csrc/s2m_icp_close.hpp (the close of an ICP iteration: Umeyama, the composition, PCL's convergence
// state machine; one source for the host loop and the device loop) built by the host compiler alone, for tests/test_icp_grid_cpu.py.
//   icp_close_main umeyama                 stdin: lines of 15 hex floats (mean_src 3, mean_tgt 3, sigma 9); stdout: T as 16 hex words
//   icp_close_main align src.bin n_src tgt.bin n_tgt max_corr_dist max_iter
//                                          a brute-force ICP on packed xyz floats whose iterations icp_close_step closes;
//                                          stdout: converged iterations, then T as 16 hex words
//   icp_close_main close                   stdin: lines of 57 numbers (hex floats, integers in decimal): the 17 sums, the incoming
//                                          IcpLoopState (T 16, T_step 16, prev_mse, it, conv, similar, done), max_iter, trans_eps,
//                                          fit_eps; stdout: the outgoing state as the 38 32-bit hex words of the struct. A state
//                                          that comes in done is not closed (k_icp_close's guard).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "s2m_icp_close.hpp"

static void print_T(const float T[16])
{
    for (int i = 0; i < 16; i++) {
        uint32_t w;
        memcpy(&w, &T[i], 4);
        printf("%08x%c", w, i == 15 ? '\n' : ' ');
    }
}

static std::vector<float> read_xyz(const char* path, size_t n)
{
    std::vector<float> v(3 * n);
    FILE* f = fopen(path, "rb");
    if (!f || fread(v.data(), sizeof(float), 3 * n, f) != 3 * n) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fclose(f);
    return v;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "umeyama")) {
        char line[1024];
        while (fgets(line, sizeof(line), stdin)) {
            float v[15];
            char* p = line;
            int k = 0;
            for (; k < 15; k++) {
                char* e;
                v[k] = (float)strtod(p, &e);
                if (e == p) break;
                p = e;
            }
            if (k < 15) continue;
            float T[16];
            s2m::host_umeyama(v, v + 3, v + 6, T);
            print_T(T);
        }
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "close")) {
        static_assert(sizeof(s2m::IcpLoopState) == 38 * sizeof(uint32_t), "printed as 38 words");
        char line[8192];
        while (fgets(line, sizeof(line), stdin)) {
            double v[57];
            char* p = line;
            int k = 0;
            for (; k < 57; k++) {
                char* e;
                v[k] = strtod(p, &e);
                if (e == p) break;
                p = e;
            }
            if (k < 57) continue;
            s2m::IcpLoopState st;
            for (int i = 0; i < 16; i++) { st.T[i] = (float)v[17 + i]; st.T_step[i] = (float)v[33 + i]; }
            st.prev_mse = v[49];
            st.it = (int)v[50]; st.conv = (int)v[51]; st.similar = (int)v[52]; st.done = (int)v[53];
            const s2m::IcpCloseParams cp = s2m::icp_close_params((int)v[54], v[55], v[56]);
            if (!st.done) s2m::icp_close_step(v, cp, &st);
            uint32_t w[38];
            memcpy(w, &st, sizeof(w));
            for (int i = 0; i < 38; i++) printf("%08x%c", w[i], i == 37 ? '\n' : ' ');
        }
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "align")) {
        const size_t ns = strtoul(argv[3], nullptr, 10), nt = strtoul(argv[5], nullptr, 10);
        std::vector<float> cur = read_xyz(argv[2], ns);
        const std::vector<float> tgt = read_xyz(argv[4], nt);
        const double max_corr = strtod(argv[6], nullptr), max_d2 = max_corr * max_corr;
        const s2m::IcpCloseParams cp = s2m::icp_close_params(atoi(argv[7]), 1e-6, 1e-6);
        s2m::IcpLoopState st;
        s2m::icp_state_init(&st);
        while (!st.done) {
            double S[17] = { 0 };
            for (size_t i = 0; i < ns; i++) {
                const float* p = &cur[3 * i];
                float bd = INFINITY;
                long bi = -1;
                for (size_t j = 0; j < nt; j++) {
                    const float dx = p[0] - tgt[3 * j], dy = p[1] - tgt[3 * j + 1], dz = p[2] - tgt[3 * j + 2];
                    const float d = (dx * dx + dy * dy) + dz * dz;
                    if (d < bd) { bd = d; bi = (long)j; }
                }
                if (bi < 0 || !((double)bd <= max_d2)) continue;
                const float* t = &tgt[3 * bi];
                S[0] += 1.0; S[1] += (double)bd;
                for (int d = 0; d < 3; d++) { S[2 + d] += p[d]; S[5 + d] += t[d]; }
                for (int r = 0; r < 3; r++)
                    for (int c = 0; c < 3; c++) S[8 + r * 3 + c] += (double)t[r] * p[c];
            }
            const int before = st.it;
            s2m::icp_close_step(S, cp, &st);
            if (st.it == before) break;
            const float* m = st.T_step;
            for (size_t i = 0; i < ns; i++) {
                float* p = &cur[3 * i];
                const float x = m[0] * p[0] + m[1] * p[1] + m[2] * p[2] + m[3];
                const float y = m[4] * p[0] + m[5] * p[1] + m[6] * p[2] + m[7];
                const float z = m[8] * p[0] + m[9] * p[1] + m[10] * p[2] + m[11];
                p[0] = x; p[1] = y; p[2] = z;
            }
        }
        printf("%d %d ", st.conv, st.it);
        print_T(st.T);
        return 0;
    }
    fprintf(stderr, "usage: icp_close_main umeyama | close | align src.bin n_src tgt.bin n_tgt max_corr_dist max_iter\n");
    return 2;
}
