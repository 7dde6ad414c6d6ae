// cn_tuning.h -- the cn_set_tuning knobs: one struct of plain ints that the launchers read, and the one
// table that states each key's number, field, default and accepted values.  A new knob is a field of
// CnTuning plus a row of CN_TUNING_KEYS (and its entry under cn_set_tuning in include/centernet_amd.h).
// Keys -1 ... 64 are closed: tests/test_tuning_host.py records exactly which of them are accepted (and that 48 is
// not a key); a new knob takes the next free number from 65 on and is documented BELOW cn_set_tuning there.
// Plain process-global ints, no locking: see the THREADING note in include/centernet_amd.h.
#pragma once

struct CnTuning {
    int nbuf, narrow, bm, nosplit, nostem, swz, setprio, dbgskip, nohalo, stem_persist, dcn_split, bm256, waves8,
        split_min_chunks, split_max, stagger_pct, occ4, f32s_lds_weights, f32s_policy, dcn_tile2d, dcn_form,
        heads_remap, heads_reg, stem16s, c3p, c3p_stagger, c3p_knobs, c3p_heads, c3p_deconv, c3p_s2, dcn_team,
        dcn_team_wgs, dcn_team_stagger, offconv, offconv_teams1, dcn_wide, dcn_wide_wgs, stem_dbg, stem_stagger,
        dcn_wide_prefetch, proj, c3p_grid, conv16h;
};
extern CnTuning cn_knobs;   // the one instance (cn_conv.hip, next to cn_set_tuning / cn_get_tuning / cn_reset_tuning)

struct CnTuningKey {
    int key;
    int CnTuning::*field;   // nullptr = retired: still accepted, has no effect, reads back 0
    int def;                // value at start and after cn_reset_tuning
    int lo, hi;             // accepted: lo ... hi,
    int n_also, also[4];    // and these values
};

constexpr CnTuningKey CN_TUNING_KEYS[] = {
    // implicit GEMM (cn_conv.hip)
    {1, &CnTuning::nbuf, 0, 0, 2},                // LDS tile buffers: 0 = per-shape default, 1 / 2 = force
    {2, &CnTuning::narrow, 0, 0, 1},              // 1 = never prefer 64-wide N tiles
    {3, nullptr, 0, 0, 0, 1, {64}},               // (retired) 128-pixel tiles of the deformable kernel
    {4, &CnTuning::bm, 0, 0, 0, 2, {64, 128}},    // 64 / 128 = force the dense pixel tile, 0 = default
    {5, &CnTuning::nosplit, 0, 0, 1},             // 1 = never split K
    {6, &CnTuning::nostem, 0, 0, 1},              // 1 = generic implicit-GEMM stem instead of cn_stem.hip
    {7, &CnTuning::swz, 0, 0, 2},                 // XCD-aware tile order: 0 = deformable kernel only, 1 = all, 2 = none
    {8, &CnTuning::setprio, 1, 0, 1},             // s_setprio(1) around the MFMA clusters (+0.9 % measured)
    {9, &CnTuning::dbgskip, 0, 0, 2047},          // ablation only: bit 0 skip A staging, bit 1 skip B staging; bits 8 / 9: probe builds of cn_dcn3 / cn_dcn4
    {10, &CnTuning::nohalo, 0, 0, 1},             // 1 = generic implicit GEMM for 3x3/s1 instead of cn_conv3x3.hip
    {11, nullptr, 0, 0, 0},                       // (retired in round 5) fp32 LDS-window deformable kernel: 20-30 % slower than the gather form
    {12, &CnTuning::stem_persist, 1, 0, 1},       // persistent, prefetching stem kernel (cn_stem.hip)
    {13, &CnTuning::dcn_split, 0, 0, 1, 2, {3, 9}},   // tap split of the deformable kernel: 0 = auto, 1 = never, 3 / 9 = force
    {16, &CnTuning::split_min_chunks, 8, 1, 64},  // K chunks per split-K slice, at least
    {17, &CnTuning::split_max, 16, 1, 64},        // split-K slices, at most
    {22, &CnTuning::dcn_tile2d, 1, 0, 1},         // deformable kernel: 1 = 8-wide pixel blocks as tiles, 0 = row segments
    // f32s deformable kernel: 0 = by shape and grid, in dcn_route's order of preference (cn_dcn.hip), 1 = global-gather
    // form always, 2 = register-sampling form (cn_dcn2.hip), 4 / 5 = team form (cn_dcn3.hip) in T / N mode, 6 / 7 = wide
    // form (cn_dcn4.hip; 7: four blocks per workgroup), each for every shape it takes (the gather form for the others)
    {23, &CnTuning::dcn_form, 0, 0, 2, 4, {4, 5, 6, 7}},
    {27, &CnTuning::stem16s, 1, 0, 1},            // f32s form of the stride-1 16-channel stem (DLA base_layer); 0 = fp32 kernel
    // LDS-halo kernel (cn_conv3x3.hip)
    {14, &CnTuning::bm256, 0, 0, 3},              // 64-wide layers on 256-pixel tiles: 1 = four waves, 2 / 3 = eight waves (f32s); no gain, measured
    {15, &CnTuning::waves8, 1, 0, 1},             // 8-wave workgroups for the 128-wide tiles
    {18, &CnTuning::stagger_pct, 100, 0, 255},    // phase shift of co-resident workgroups, percent of one tile's MFMA time (0 = off)
    {19, &CnTuning::occ4, 0, 0, 2},               // 4-workgroups-per-CU form of the 64-wide tiles: 0 = by rounds rule, 1 = always, 2 = never
    {20, &CnTuning::f32s_lds_weights, 1, 0, 1},   // f32s 128-wide tiles: 1 = per-tap weight tile in LDS, 0 = register-streamed weights
    {21, &CnTuning::f32s_policy, 0, 0, 7},        // (A/B) bit 0 = 128-wide tiles as eight waves three taps ahead, bit 1 = 64-wide tiles two taps ahead, bit 2 = 8 x 16 tiles everywhere
    {24, &CnTuning::heads_remap, 1, 0, 3},        // (A/B) bit 0 = fused heads, bit 1 = multi-block Cout, on a 1-D row-interleaved grid
    {26, &CnTuning::heads_reg, 1, 0, 3},          // (A/B) fused f32s heads with the hidden layer in registers
    // persistent 3x3 kernel (cn_conv3x3p.hip)
    {28, &CnTuning::c3p, 1, 0, 7},                // 0 = off, 1 = on for the shapes it takes, >= 2 = also launches of < 256 work items
    // start delay of the second resident workgroup, in units of 256 cycles (64 was worth 1-2 % with the
    // unpipelined schedule; with the pipelined one 0 is: r05_c3p_pipe.txt)
    {29, &CnTuning::c3p_stagger, 0, 0, 255},
    {30, &CnTuning::c3p_knobs, 2, 0, 255},        // (A/B) see P3Args.knobs
    {31, &CnTuning::c3p_heads, 1, 0, 1},          // the fused heads (hidden width 64) on this kernel; 0 = halo kernel
    {32, &CnTuning::c3p_deconv, 1, 0, 1},         // ConvTranspose2d(4, 2, 1) in parity form on this kernel; 0 = halo kernel
    {33, &CnTuning::c3p_s2, 1, 0, 1},             // 3x3 / stride 2 / pad 1 in parity-plane form on this kernel; 0 = implicit GEMM
    // workgroups per XCD of a launch, at most (64 = two per CU).  For tests: a smaller cap gives every workgroup
    // several items at shapes whose float64 reference is cheap (tests/test_gpu_c3p_items.py)
    {47, &CnTuning::c3p_grid, 64, 1, 64},
    // team form of the deformable kernel (cn_dcn3.hip)
    // 0 = off, 1 = layers with <= 64 output channels, 2 = every layer it takes (T mode), 3 = every layer, N mode
    // where Cout is a multiple of 128 and that still fills the chip
    {36, &CnTuning::dcn_team, 3, 0, 3},
    {37, &CnTuning::dcn_team_wgs, 512, 1, 4096},  // K split until a launch has this many workgroups
    // start delay of the second resident workgroup of every CU, in units of 256 cycles (sweep 0 .. 128 at B = 32:
    // 32-64 is 5-9 % faster on the multi-round shapes, nothing on the others; profiles/r05_dcn_team_stagger.txt)
    {38, &CnTuning::dcn_team_stagger, 32, 0, 1024},
    // offset / mask convolution (cn_offconv.hip)
    {39, &CnTuning::offconv, 1, 0, 1},            // 0 = off (the LDS-halo kernel takes these layers)
    {40, &CnTuning::offconv_teams1, 768, 0, 1000000},   // workgroups from which the four-wave form is used
    // wide form of the deformable kernel (cn_dcn4.hip)
    {41, &CnTuning::dcn_wide, 1, 0, 1},           // 0 = off, 1 = layers with Cout % 128 == 0 that the form takes
    {42, &CnTuning::dcn_wide_wgs, 256, 1, 4096},  // K split until a launch has this many workgroups
    {45, &CnTuning::dcn_wide_prefetch, 1, 0, 1},  // L2 prefetch of the weight slabs three steps ahead
    // stem + max-pool kernel (cn_stem.hip), measurement only
    {43, &CnTuning::stem_dbg, 0, 0, 31},          // probe switches (StemArgs.dbg)
    {44, &CnTuning::stem_stagger, 0, 0, 1024},    // start delay of the second resident workgroup, units of 256 cycles
    // 1x1 projections (cn_proj.hip)
    {46, &CnTuning::proj, 1, 0, 1},               // 1 = f32s 1x1 layers without residual on this kernel, 0 = implicit GEMM
    // 16-channel 3x3 kernel (cn_conv16.hip)
    {65, &CnTuning::conv16h, 1, 0, 1},            // 1 = fp16 layers it takes on its half form, 0 = halo kernel / implicit GEMM
};

constexpr CnTuning cn_tuning_defaults()
{
    CnTuning t = {};
    for (const CnTuningKey &k : CN_TUNING_KEYS)
        if (k.field) t.*k.field = k.def;
    return t;
}
