// Prints the frame-tile table evc::frame_tiles (evc_internal.h) builds, for tests/test_solve_common_host.py.  Host code only:
// no HIP call, no device; build with `hipcc --offload-host-only` (add -fsanitize=address,undefined for a sanitizer run: every
// array is allocated at exactly the size the table needs).
//
//   solve_common_host_main F:T:o0,o1,...,on  ...      (F:T:- for a call without utt_offsets)
//
// Per argument four lines: "n_tiles cap counted", the tiles as x y z w quadruples, utt_tile0, utt_frames.
#include "../exemplars_vc_amd/csrc/evc_internal.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        char* p = argv[a];
        const int F = (int)strtol(p, &p, 10);
        const int T = (int)strtol(p + 1, &p, 10);
        std::vector<int> offs;
        if (strcmp(p, ":-") != 0)
            while (*p) offs.push_back((int)strtol(p + 1, &p, 10));
        const int* off = offs.empty() ? nullptr : offs.data();
        const int n_utt = offs.empty() ? 1 : (int)offs.size() - 1;
        const int counted = evc::frame_tiles(F, off, n_utt, T, nullptr, nullptr, nullptr);
        int4* tiles = new int4[counted];
        int* tile0 = new int[n_utt + 1];
        int* frames = new int[n_utt];
        const int n = evc::frame_tiles(F, off, n_utt, T, tiles, tile0, frames);
        printf("%d %d %d\n", n, evc::frame_tile_cap(T, F, n_utt), counted);
        for (int t = 0; t < n; ++t) printf("%d %d %d %d ", tiles[t].x, tiles[t].y, tiles[t].z, tiles[t].w);
        printf("\n");
        for (int u = 0; u <= n_utt; ++u) printf("%d ", tile0[u]);
        printf("\n");
        for (int u = 0; u < n_utt; ++u) printf("%d ", frames[u]);
        printf("\n");
        delete[] tiles;
        delete[] tile0;
        delete[] frames;
    }
    return 0;
}
