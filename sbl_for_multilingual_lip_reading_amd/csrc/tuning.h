// Process-wide settings of the launchers and the settled dispatch thresholds, each with the measurement that decided it
// (DESIGN.md has the history).  The thresholds were run-time A/B switches once; the losing sides are gone.
#pragma once

// Matrix-product precision of the tile engine (sbl_set_matmul_precision, gemm.hip): 0 = fp32 MFMA, 6 / 3 / 1 = bf16 MFMA terms.
extern int g_sbl_prec;

// The two routing switches of sbl_set_tuning (conv.hip).  Both sides of each are shipped kernels: the patch-resident ones take
// the large 3x3 / stride-1 maps, the implicit-GEMM / position-major ones everything else, and the suite uses the switches to
// run the latter on the large maps too.
struct SblRouting {
    int conv_patch;            // knob 5: 2 = patch-resident forward / input gradient (conv_patch.h), 0 = the per-tap gather kernels
    int conv_patch_wgrad;      // knob 9: smallest map (pixels) that takes the patch-resident weight gradient (conv_patch_wgrad.h), 0 = never
                               // (same-box step A/B 0 / 100 / 30: 32.22 / 31.84 / 31.73 ms)
};
extern SblRouting g_sbl_route;

// ---- dense products (gemm.hip, mfma_gemm.h)
constexpr int sbl_big_min_tiles = 4096;          // 64x64-tile count from which dense products take 128x128 tiles (4352x2048x512: 128x128
                                                 // tiles 131 us, 64x64 115 us; 2048 / 1024 here: step +0.1 / +0.3 ms)
constexpr int sbl_wave_ksplit_max_tiles = 320;   // largest tile count that takes the wave-group K split (same-box A/B of the whole
                                                 // step: 0 -> 32.99, 320 -> 32.81, 768 -> 32.99 ms)
// in-launch split-K of the two-direction decoder products (sbl_gemm2_f32): launches below this many tiles split, aiming at this
// many workgroups, at most this many ways (target 128 / 256 / 512: 30.40 / 30.34 / 30.52 ms; up to 16 splits: 30.56; splitting
// the 192-640-tile launches too, targets 512 / 1024: 32.77 / 31.22 against 31.07 ms)
constexpr int sbl_gemm2_split_tiles = 192, sbl_gemm2_split_target = 256, sbl_gemm2_split_max = 8;
// row-starved two-direction products (sbl_gemm2_rows_f32): a launch whose 32x32 tiling would give fewer than this many
// workgroups (2 * cdiv(M, 32) * cdiv(N, 32)) takes 16x16 tiles (sbl_skinny16_gemm_kernel) instead
// (same-box step A/B, parent / this value, three interleaved runs each: 30.161, 30.262, 30.177 / 29.908, 29.939, 29.812 ms;
// kernel trace: K = 2048 launches 29.0 -> 14.9 us, the moved K = 512 ones 10.0 -> 6.4 us.  Only this value was run in the step.)
constexpr int sbl_rows16_max_wgs32 = 256;
// ... and at most this many rows per direction: sbl_gemm2_f32's bound for its 32x32 skinny kernel (max_m), whose sums the 16x16
// kernel repeats term by term.  Above it the K = 2048 products come from the tiled split-K route, and moving them (M = 144...224,
// the optional second step) changes their rounding: with dropout on, the two row layouts of the last decoder layer then differ
// by 1.4 x the bound that tests/test_decoder_last_layer_rows_gpu.py holds them to (f32, alternating coins)
constexpr int sbl_rows16_max_m = 128;
// ... its register stages: 4 16-deep groups per range and stage from this K on (K = 2048: a range is 256 deep, half of it in
// flight per stage), 2 below (K = 512: both stages together hold a whole 64-deep range)
constexpr int sbl_rows16_deep_k = 1024;

// ---- trunk convolutions (conv.hip, conv_patch_wgrad.h)
constexpr int sbl_pm_max_hw = 121;               // largest Ho*Wo of a 3x3 / stride-1 convolution that takes the position-major path (ResNet
                                                 // layers 2-4: 11x11, 6x6, 3x3; the 22x22 maps of layer 1 lose: 6 % padding, 434 vs 396 us)
constexpr bool sbl_wg_s2_small = true;           // stride-2 weight gradients on 64x64 tiles (128 -> 256: 459 -> 335 us, 256 -> 512: 447 -> 400 us)
constexpr int sbl_wg_s2_target = 1536;           // ... and their workgroup target (same-box step A/B 32.44 / 32.34 / 32.29 ms for 128-tiles /
                                                 // 64-tiles / 64-tiles + 1536)
constexpr int sbl_pm_wg64_max_m = 512;           // position-major weight gradients with Cout <= this on 64x64 tiles (same-box step A/B
                                                 // always 128x128 / 128 / 256 / 512: 32.33 / 32.32 / 32.33 / 32.20 ms)
constexpr int sbl_patch_wgrad_cus = 256;         // workgroups of the patch-resident weight gradient: one per CU (leaving CUs to the other
                                                 // stream, 224 / 192 / 128: 31.88 / 31.85 / 32.06 against 31.92 ms: noise)
