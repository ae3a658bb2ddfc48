// path_table - prints the sampler's path decision (csrc/dsd_path.hpp) as canonical text, one line per input.
//   path_table                                              the fixed grid of tests/golden/path_decisions.json
//   path_table n_cu L B T loop lat tile conv split graph off   that one input
// Host-only: g++ -std=c++17 tests/path_table.cpp (tests/test_path_decisions.py builds and runs it).
#include <cstdio>
#include <cstdlib>

#include "../diffsinger_amd/csrc/dsd_path.hpp"

using namespace dsd;

static const char* kind_name(PathKind k) {
    switch (k) {
        case PathKind::PersistentWino: return "persistent-winograd";
        case PathKind::PersistentDirect: return "persistent-direct";
        case PathKind::PersistentSplit: return "persistent-split";
        case PathKind::Latency: return "latency";
        default: return "per-layer";
    }
}

static void row(int n_cu, int L, int B, int T, int loop, int lat, int tile, int conv, int split, int graph, int off) {
    PathInput in{};
    in.n_cu = n_cu; in.B = B; in.ntile32 = (T + 31) / 32; in.L = L;
    in.loop_mode = loop; in.lat_req = lat; in.layer_tile_req = tile; in.conv_mode = conv;
    in.has_w1w = true;                   // packed with the weights, which a prepared batch always has
    in.split_mode = split != 0; in.use_graph = graph != 0; in.persist_off = off != 0;
    const SamplerPath p = sampler_path(in);
    std::printf("n_cu=%d L=%d B=%d T=%d loop=%d lat=%d tile=%d conv=%d split=%d graph=%d off=%d -> %s G=%d frames=%d lat_wino=%d upc=%d launches=%d key=%d\n",
                n_cu, L, B, T, loop, lat, tile, conv, split, graph, off, kind_name(p.kind), p.G, p.layer_frames, p.lat_wino ? 1 : 0,
                p.utt_per_chunk, p.launches, p.graph_tile);
}

int main(int argc, char** argv) {
    if (argc == 12) {
        int a[11];
        for (int i = 0; i < 11; ++i) a[i] = std::atoi(argv[i + 1]);
        row(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10]);
        return 0;
    }
    if (argc != 1) {
        std::fprintf(stderr, "usage: path_table [n_cu L B T loop lat tile conv split graph off]\n");
        return 2;
    }
    const int n_cus[] = {4, 8, 64, 256}, Ls[] = {20, kLoopMaxLayers + 1}, Bs[] = {1, 2, 3, 5, 8, 16, 32};
    const int Ts[] = {32, 512, 777, 1024, 1550, 2048, 4200, 5000, 8224}, lats[] = {-1, 0, 2, 4, 8, 16}, tiles[] = {0, 32, 64};
    for (int n_cu : n_cus)
        for (int L : Ls)
            for (int B : Bs)
                for (int T : Ts)
                    for (int loop = 0; loop < 4; ++loop)
                        for (int lat : lats)
                            for (int tile : tiles)
                                for (int conv = 0; conv < 2; ++conv)
                                    for (int split = 0; split < 2; ++split)
                                        for (int graph = 0; graph < 2; ++graph)
                                            for (int off = 0; off < 2; ++off) row(n_cu, L, B, T, loop, lat, tile, conv, split, graph, off);
    return 0;
}
