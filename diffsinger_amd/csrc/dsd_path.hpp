// dsd_path.hpp - which kernels a prepared batch runs on.  Host-only, plain C++17, no HIP: dsd.hip fills a PathInput from the handle and every
// launch site and getter reads the one SamplerPath computed from it; tests/path_table.cpp prints the decision for a grid of inputs
// (tests/golden/path_decisions.json).
#pragma once
#include <algorithm>

namespace dsd {

constexpr int kLoopMaxLayers = 64;      // layers a persistent loop's parameter block holds (LoopParams::dil, dsd_loop.hpp)

struct PathInput {
    int n_cu;               // workgroups that are certainly co-resident at 1 per CU
    int B, ntile32;         // utterances of the prepared batch, 32-frame tiles per utterance
    int L;                  // residual layers
    int loop_mode;          // 0 per-layer kernels, 1 persistent loop, 2 automatic, 3 latency kernels (dsd_set_loop_mode)
    int lat_req;            // -1 by batch size, 0 never, 2 / 4 / 8 / 16 forced (dsd_set_lat_split)
    int layer_tile_req;     // 0 auto, 32, 64 (dsd_set_layer_tile)
    int conv_mode;          // 1 Winograd F(2,3), 0 direct (dsd_set_conv_mode)
    bool has_w1w;           // the transformed convolution weights are packed
    bool split_mode, use_graph, persist_off;
};

enum class PathKind { PersistentWino, PersistentDirect, PersistentSplit, Latency, PerLayer };

struct SamplerPath {
    PathKind kind;          // what the K-step loops (dsd_sample_ddpm / dsd_sample_plms) run
    int G;                  // row split of the latency kernels, 0 = the per-layer kernel (also what a single evaluation, dsd_denoise, runs)
    int layer_frames;       // frames per workgroup of the per-layer kernel: 32 or 64
    bool lat_wino;          // the latency kernels' convolution node is the Winograd form (k_lat_conv_w)
    int utt_per_chunk;      // persistent loop: whole utterances per launch ...
    int launches;           // ... and launches per call; both 0 on the other paths
    int graph_tile;         // distinguishes the cached graphs of one (kind, B, T, k_step, interval) by the kernels their nodes hold
    bool persistent() const { return kind == PathKind::PersistentWino || kind == PathKind::PersistentDirect || kind == PathKind::PersistentSplit; }
    bool winograd() const { return kind == PathKind::PersistentWino || lat_wino; }      // the dilated convolution runs as Winograd F(2,3)
};

inline SamplerPath sampler_path(const PathInput& in) {
    const int ntiles = in.B * in.ntile32, n_cu = in.n_cu;
    const bool wino = in.conv_mode == 1 && in.has_w1w;
    SamplerPath r{};

    // Row split G of the latency kernels for the prepared batch, 0 = not on that path.  Automatic mode: the largest G in {16, 8, 4, 2} that
    // still gives every workgroup a CU of its own - i.e. batches that leave at least half of the chip idle - and G = 8 for the band above it
    // (between half and 5/8 of the CU count in tiles: 129-160 on 256 CUs, e.g. ONE phrase of 4200-5000 frames or 5 x 1024): the persistent loop
    // leaves 37-50 % of the CUs without a tile there, 8 x ntiles workgroups in at most five grid waves measured 115-121 ms against its 127 ms
    // per K = 100 call (profiles/r47_midsize_paths.jsonl); one more grid wave (163 tiles) and the loop wins again.
    if (!(in.split_mode || in.layer_tile_req || in.lat_req == 0 || in.loop_mode < 2)) {
        int g = (16 * ntiles <= n_cu) ? 16 : (8 * ntiles <= n_cu) ? 8 : (4 * ntiles <= n_cu) ? 4 : (2 * ntiles <= n_cu) ? 2 : 0;
        // (the band exists for the DIRECT-convolution loop only: the Winograd loop takes 104 ms per launch and wins it back - profiles/r5_03_shape_sweep.jsonl)
        if (g == 0 && in.loop_mode == 2 && !wino && ntiles < n_cu && 8 * ntiles <= 5 * n_cu) g = 8;
        if (in.loop_mode == 3 && g == 0) g = 2;
        if (g && (in.lat_req == 2 || in.lat_req == 4 || in.lat_req == 8 || in.lat_req == 16)) g = in.lat_req;
        r.G = g;
    }
    // the Winograd form of the convolution for G = 2 / 4 / 8 (4 x 777: 71.0 ms against 81.9, 1 x 1550: 45.3 against 50.2, 1 x 1000: 31.2 against 32.0);
    // at G = 16 a wave's share is 128 short MFMAs and the direct kernel with its own packing stays ahead (24.6 ms against 25.0; profiles/r5_11_*)
    r.lat_wino = wino && r.G && r.G != 16;

    // The split-precision layer kernel and the latency kernels exist for 32-frame tiles only.  Otherwise 32-frame workgroups until there are
    // enough of them to keep two resident per CU on all 256 CUs; beyond that 64-frame workgroups halve the weight traffic out of L2 per frame.
    r.layer_frames = (in.split_mode || r.G) ? 32 : in.layer_tile_req ? in.layer_tile_req : (ntiles > 1024) ? 64 : 32;
    r.graph_tile = r.layer_frames / 32 + 100 * r.G + 10000 * (wino ? 1 : 0);      // (the latency nodes differ by convolution form)

    // The persistent loop: 32-frame tiles, a whole utterance fits the co-resident grid (ntile32 = 0: no batch is prepared yet)
    bool loop = (in.loop_mode == 1 || in.loop_mode == 2) && !in.persist_off && in.use_graph && r.layer_frames == 32 && n_cu >= 8 &&
                in.ntile32 >= 1 && in.ntile32 <= n_cu && in.L <= kLoopMaxLayers && !(in.loop_mode == 2 && r.G);
    if (loop) {
        // chunks of whole utterances, at most one workgroup per CU (all workgroups of a launch wait for each other)
        r.utt_per_chunk = std::max(1, n_cu / in.ntile32);
        r.launches = (in.B + r.utt_per_chunk - 1) / r.utt_per_chunk;
        if (in.loop_mode == 2) {
            // chunks of whole utterances may leave much of the chip idle (T = 5000: 157 tiles per launch on 256 CUs); the per-layer kernels
            // have no such constraint, only the wave quantisation of their grid, and cost ~5 % more at equal occupancy
            const double u_p = (double)ntiles / ((double)r.launches * n_cu);
            // (the per-layer kernels evaluate the direct convolution: at equal occupancy they take 1.05 x the direct loop's time and 1.29 x the
            // Winograd loop's - 133 ms against 127 / 103.7 ms per 256 tiles)
            const double rel = (wino && !in.split_mode) ? 0.78 : 0.95;
            const double u_l = rel * (double)ntiles / ((double)((ntiles + n_cu - 1) / n_cu) * n_cu);
            if (u_l > u_p) loop = false;
        }
    }
    if (!loop) r.utt_per_chunk = r.launches = 0;
    // (the persistent loop evaluates the dilated convolution as Winograd F(2,3), dsd_loop_wino.hpp, unless the direct form or split precision is chosen)
    r.kind = !loop ? (r.G ? PathKind::Latency : PathKind::PerLayer)
                   : in.split_mode ? PathKind::PersistentSplit : wino ? PathKind::PersistentWino : PathKind::PersistentDirect;
    return r;
}

}  // namespace dsd
