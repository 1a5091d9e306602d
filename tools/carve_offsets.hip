// Prints where the workspace carvers of the learn entries (and of the cd / beta solves they build on) put every
// sub-array, as byte offsets from the caller's pointer, for a pointer at a multiple of 256 bytes and for one 8 bytes
// past it, and the byte counts.  A host program with no device work: it includes ONE translation unit of the library
// (the carvers are local to theirs) and links the rest from libevc_hip.so.  Build it once per unit and compare the four
// outputs across two commits; a change of the carving code must leave them identical.
//
//   for u in LEARN CD BETA BETA_LEARN; do
//     hipcc --offload-arch=gfx950 -O1 -std=c++17 -DCARVE_$u tools/carve_offsets.hip -o carve_$u \
//           -Lexemplars_vc_amd -levc_hip -Wl,-rpath,$PWD/exemplars_vc_amd   # optional: -Xarch_host -fsanitize=address,undefined
//     ./carve_$u
//   done
// (The carvers of the main solve are in a header of their own, csrc/evc_solve_plan.h: tests/solve_plan_host_main.hip.)
#if defined(CARVE_LEARN)
#include "../exemplars_vc_amd/csrc/evc_learn.hip"
#elif defined(CARVE_CD)
#include "../exemplars_vc_amd/csrc/evc_cd.hip"
#elif defined(CARVE_BETA)
#include "../exemplars_vc_amd/csrc/evc_beta.hip"
#elif defined(CARVE_BETA_LEARN)
#include "../exemplars_vc_amd/csrc/evc_beta_learn.hip"
#else
#error "define one of CARVE_LEARN, CARVE_CD, CARVE_BETA, CARVE_BETA_LEARN"
#endif

#include <stdio.h>

using namespace evc;

static char* g_ws;
static void head(const char* what, int M, int R, int T, int esize, size_t bytes) {
    printf("%s M=%d R=%d T=%d esize=%d ws%%256=%d bytes=%zu:", what, M, R, T, esize, (int)((uintptr_t)g_ws % 256), bytes);
}
#define OFF(p) printf(" " #p "=%td", reinterpret_cast<char*>(p) - g_ws)

template <typename T> static void one(int M, int R, int T_) {
    const int es = (int)sizeof(T);
#if defined(CARVE_LEARN)
    if (M > LEARN_MAX_M || R > LEARN_MAX_R) return;
    const auto w = carve_learn<T>(g_ws, make_dims(es, M, R, T_, 1, 0));
    head("carve_learn", M, R, T_, es, w.bytes);
    OFF(w.Xt); OFF(w.Am); OFF(w.Ht); OFF(w.Vt); OFF(w.part); OFF(w.err2); OFF(w.ring); OFF(w.solve_ws);
#elif defined(CARVE_CD)
    if (M > CD_MAX_M || R > CD_LEARN_MAX_R) return;
    for (int n_utt = 1; n_utt <= 3; n_utt += 2) {
        const auto c = carve_cd<T>(g_ws, cd_geometry(M), R, T_, n_utt);
        head(n_utt == 1 ? "carve_cd" : "carve_cd(3 utt)", M, R, T_, es, c.bytes);
        OFF(c.Ac); OFF(c.Gb); OFF(c.hess); OFF(c.R); OFF(c.tiles); OFF(c.utt_tile0); OFF(c.part); OFF(c.stop); OFF(c.vinit);
        OFF(c.trace);
        printf("\n");
    }
    for (int S = 1; S <= LEARN_MAX_SPLITS; S *= 8) {
        const auto w = carve_cd_learn<T>(g_ws, M, R, T_, S);
        head(S == 1 ? "carve_cd_learn S=1" : S == 8 ? "carve_cd_learn S=8" : "carve_cd_learn S=64", M, R, T_, es, w.bytes);
        OFF(w.cd); OFF(w.Xt); OFF(w.Ht); OFF(w.partP); OFF(w.partG); OFF(w.G); OFF(w.P); OFF(w.Gb); OFF(w.hess); OFF(w.dpart);
        OFF(w.ring);
        if (S < LEARN_MAX_SPLITS) printf("\n");
    }
#elif defined(CARVE_BETA)
    if (M > BETA_MAX_M) return;
    for (int n_utt = 1; n_utt <= 3; n_utt += 2) {
        const auto w = carve_beta<T>(g_ws, M, R, T_, n_utt);
        head(n_utt == 1 ? "carve_beta" : "carve_beta(3 utt)", M, R, T_, es, w.bytes);
        OFF(w.Ap1); OFF(w.Ap3); OFF(w.Xp); OFF(w.errf); OFF(w.tiles); OFF(w.utt_tile0); OFF(w.utt_frames); OFF(w.stop);
        OFF(w.h0); OFF(w.einit); OFF(w.eprev); OFF(w.trace);
        if (n_utt == 1) printf("\n");
    }
#else
    if (M > BETA_MAX_M || R > LEARN_MAX_R) return;
    const auto w = carve_bl<T>(g_ws, make_dims(es, M, R, T_, 1));
    head("carve_bl", M, R, T_, es, w.bytes);
    OFF(w.Xt); OFF(w.Am); OFF(w.Ht); OFF(w.Vt); OFF(w.Q2t); OFF(w.part); OFF(w.beta_ws);
#endif
    printf("\n");
}

int main() {
    static const int shapes[][3] = {{1, 1, 1}, {25, 17, 70}, {50, 24, 150}, {50, 512, 65536}, {201, 20, 6880}, {513, 16, 40},
                                    {528, 4096, 40}, {1024, 1024, 40}, {1056, 16, 40}};
    for (int shift = 0; shift <= 8; shift += 8) {
        g_ws = reinterpret_cast<char*>(uintptr_t(1) << 40) + shift;      // never dereferenced
        for (const auto& sh : shapes) {
            one<double>(sh[0], sh[1], sh[2]);
            one<float>(sh[0], sh[1], sh[2]);
        }
    }
    return 0;
}
