// ResNet-18 trunk convolutions as NHWC implicit GEMM on the fp32 MFMA tile engine
// (SBL/transformer/video_frontend.py:10-12 conv3x3, :69-70 1x1/stride-2 shortcut).
//   fwd   : y[pix, co]            = sum_{tap,ci} x[gather(pix,tap), ci] * w[co, tap, ci]      (+ BN stats)
//   dgrad : dx[pix, ci]           = sum_{tap,co} dy[gather'(pix,tap), co] * wt[ci, tap, co]
//   wgrad : dw[co, (tap,ci)]      = sum_{pix}    dy[pix, co] * x[gather(pix,tap), ci]         (split-K atomics)
#include "mfma_gemm.h"
#include "conv_patch.h"
#include "conv_patch_wgrad.h"

SblRouting g_sbl_route = {2, 30};
extern "C" int sbl_set_tuning(int knob, int value) {
    SBL_REQUIRE(knob == 5 || knob == 9, "sbl_set_tuning: no knob %d; the two that remain are 5 (patch-resident 3x3 / stride-1 forward / input gradient: 2 on, "
                "0 the per-tap gather kernels) and 9 (smallest map in pixels that takes the patch-resident weight gradient, 0 = never)", knob);
    if (knob == 5) {
        SBL_REQUIRE(value == 0 || value == 2, "sbl_set_tuning: knob 5 takes 2 (patch-resident kernels) or 0 (per-tap gather kernels), not %d", value);
        g_sbl_route.conv_patch = value;
    } else {
        SBL_REQUIRE(value >= 0, "sbl_set_tuning: negative value");
        g_sbl_route.conv_patch_wgrad = value;
    }
    return 0;
}

static int check_conv(const char* who, int NIMG, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    SBL_REQUIRE(NIMG > 0 && H > 0 && W > 0, "%s: bad image dims %d %d %d", who, NIMG, H, W);
    SBL_REQUIRE(Cin % 16 == 0 && Cout % 16 == 0 && Cin >= 16 && Cout >= 16, "%s: Cin=%d Cout=%d must be multiples of 16", who, Cin, Cout);
    SBL_REQUIRE((KH == 3 && KW == 3 && pad == 1) || (KH == 1 && KW == 1 && pad == 0), "%s: only 3x3/pad1 and 1x1/pad0 (got %dx%d pad %d)", who, KH, KW, pad);
    SBL_REQUIRE(stride == 1 || stride == 2, "%s: stride %d", who, stride);
    SBL_REQUIRE(sbl_fits_u32((long)NIMG * H * W * (long)(Cin > Cout ? Cin : Cout)), "%s: tensor spans more than 2 GiB (buffer descriptor range)", who);
    SBL_REQUIRE((long)NIMG * H * W < (1L << 24) && Cin < (1 << 16) && Cout < (1 << 16), "%s: more than 2^24 pixels (24-bit index arithmetic in the gathers)", who);
    return 0;
}
static inline int out_dim(int H, int K, int stride, int pad) { return (H + 2 * pad - K) / stride + 1; }

// Position-major path for 3x3 / stride-1 convolutions on small maps (sbl_pm_max_hw, tuning.h).  Its forward / input-gradient
// tiles are always 64x64: the tiles are uneven (4 / 6 / 9 taps) and co-resident, so small tiles balance best (against the
// ordinary launches' rule: layer 4 forward 400 -> 307 us, 128 TF of algorithmic FLOPs, input gradient 431 -> 324 us; layer 2
// 352 -> 327 us).
static inline bool conv_pm_ok(int Ho, int Wo, int KH, int stride) { return KH == 3 && stride == 1 && Ho * Wo <= sbl_pm_max_hw; }

constexpr int kConvWsCounters = 4096;      // same workspace convention as sbl_gemm_f32: int counters, then fp32 slabs

// ------------------------------------------------------------------ the tile rule
// Forward, input gradient and the parity-class launch choose among three tiles.  All tiles are co-resident (<= 4 workgroups
// per CU), so the launch lasts as long as the fullest CU: pick the largest tile whose count per CU (256 CUs) does not round
// up by more than ~20 % (522 128x128 tiles = 2.04/CU would run at 3/CU speed; 1044 128x64 tiles = 4.08/CU at 5/CU).
// (A 256x64 tile with 4x1 wavefronts of 64x64 was measured slower than 128x64 on the 64-channel layer: 442 vs 405 us.)
//   t128, t128x64  the launch's tile counts at 128x128 and 128x64 (the class launch sums them over its classes);
//   waste_rule     forward and plain input gradient: 512-1023 128x128 tiles that round up by more than 25 % go to 128x64;
//   no128          input gradients with the fused statistics epilogue: the 128x128 tile needs > 168 registers with it
//                  (one wave per SIMD), 128x64 instead.
enum ConvTile { kTile128x128, kTile128x64, kTile64x64 };
static ConvTile conv_tile(int N, long t128, long t128x64, bool waste_rule, bool no128) {
    const bool waste128 = waste_rule && N >= 128 && t128 >= 512 && t128 < 1024 && (double)(sbl_cdiv(t128, 256) * 256) / (double)t128 > 1.25;
    const bool skip128 = waste128 || no128;
    if (N >= 128 && t128 >= 512 && !skip128) return kTile128x128;
    if ((N < 128 || skip128) && t128x64 >= 512) return kTile128x64;
    return kTile64x64;
}
static inline int conv_tile_m(ConvTile t) { return t == kTile64x64 ? 64 : 128; }
static inline int conv_tile_n(ConvTile t) { return t == kTile128x128 ? 128 : 64; }
// fn(sbl_int<BM>{}, sbl_int<BN>{}) of the tile
template <class F>
static auto with_tile(ConvTile t, F&& fn) {
    switch (t) {
        case kTile128x128: return fn(sbl_int<128>{}, sbl_int<128>{});
        case kTile128x64: return fn(sbl_int<128>{}, sbl_int<64>{});
        default: return fn(sbl_int<64>{}, sbl_int<64>{});
    }
}

// ------------------------------------------------------------------ epilogues
// The output row map of EpiStore (mfma_gemm.h): cmap 0 = GEMM row m is output row m, 1 = parity class, 2 = position-major.
struct RowMap { int cmap, ca, cb, cH, cW, cph, cpw; };
static const RowMap kRowsDirect{0, 0, 0, 0, 0, 0, 0};
static inline RowMap rows_pm(int NIMG, int HW) { return RowMap{2, NIMG, HW, 0, 0, 0, 0}; }

// What may ride on an input-gradient convolution's epilogue (all optional):
//   addend      the residual branch's gradient, added before the store: laid out like dx (identity shortcut), or - stride-2
//               convolutions, add_class00 - the compact (NIMG, ceil(H/2), ceil(W/2), Cin) gradient of the 1x1 / stride-2
//               downsample branch, which lives on the even/even pixels only (the rows of parity class (0,0));
//   y,x,mean,inv the BatchNorm whose output gradient dx is (dx = d relu(bn(.)) of the producing block): its two backward
//               sums over g = dx * (y > 0);  x2,mean2,inv2: a second BatchNorm fed by the same y (that block's
//               downsample branch): sums[2C..4C) = (sum g, sum g * xhat2).
struct DgradFuse {
    const float* addend;
    int add_class00;
    const float* y;
    const float* x;
    const float* mean;
    const float* inv;
    const float* x2;
    const float* mean2;
    const float* inv2;
    double* sums;
    int sums_zeroed;       // the caller hands over zeros (one pooled memset per step instead of one per convolution)
};

static EpiStore<0, false> epi_plain(float* C, int N, const RowMap& r) {
    return {C, (long)N, nullptr, 0, nullptr, nullptr, 0, r.cmap, r.ca, r.cb, r.cH, r.cW, r.cph, r.cpw};
}
// + per-channel sum / sum of squares (training BatchNorm statistics of the forward)
static EpiStore<0, true> epi_stats(float* C, int N, double* stats, const RowMap& r) {
    return {C, (long)N, nullptr, 0, stats, nullptr, 0, r.cmap, r.ca, r.cb, r.cH, r.cW, r.cph, r.cpw};
}
// + addend (add_ld: EpiStore::add_ld) and, SUMS, the BatchNorm backward sums of f; without SUMS only the addend travels
template <bool SUMS>
static EpiStore<0, SUMS, true> epi_fused(float* C, int N, const DgradFuse& f, const float* add, long add_ld, const RowMap& r) {
    const DgradFuse b = SUMS ? f : DgradFuse{};
    return {C, (long)N, nullptr, 0, b.sums, nullptr, 0, r.cmap, r.ca, r.cb, r.cH, r.cW, r.cph, r.cpw,
            b.y, b.x, b.mean, b.inv, b.x2, b.mean2, b.inv2, add, add_ld};
}
// forward: statistics or not; fn(epilogue)
template <class F>
static auto with_fwd_epi(float* y, int N, double* stats, const RowMap& r, F&& fn) {
    if (stats) return fn(epi_stats(y, N, stats, r));
    return fn(epi_plain(y, N, r));
}
// input gradient: sums (+ addend), addend only, or plain.  One launch may need several epilogues of the chosen flavour (one per
// parity class, each with its row map and addend), so fn gets their maker: make(row map, addend, add_ld) -> epilogue.
template <class F>
static auto with_dgrad_epi(float* dx, int N, const DgradFuse& f, F&& fn) {
    if (f.sums) return fn([&](const RowMap& r, const float* add, long add_ld) { return epi_fused<true>(dx, N, f, add, add_ld, r); });
    if (f.addend) return fn([&](const RowMap& r, const float* add, long add_ld) { return epi_fused<false>(dx, N, f, add, add_ld, r); });
    return fn([&](const RowMap& r, const float*, long) { return epi_plain(dx, N, r); });
}

// ------------------------------------------------------------------ launches shared by forward and input gradient
// The tail split (mfma_gemm.h: two launches, two stamp slots) where it applies, else one plain launch.
template <class AL, class BL, class EPI, int BM, int BN>
static void launch_tailsplit_or_plain(const AL& al, const BL& bl, const EPI& e, int M, int N, int K, int kid, void* ws, long ws_bytes,
                                      hipStream_t s) {
    if (sbl_launch_gemm_tailsplit<AL, BL, EPI, BM, BN, 1>(al, bl, e, M, N, K, s, kid, ws, ws_bytes, kConvWsCounters)) {
        sbl_note_route(2, sbl_route_tile(BM, BN), 0, 0);
        return;
    }
    sbl_note_route(1, sbl_route_tile(BM, BN), 0, 0);
    SplitCtl sc{nullptr, nullptr, nullptr, sbl_next_stamp_slot(kid)};
    sbl_launch_gemm<AL, BL, EPI, BM, BN, 1, 2>(al, bl, e, M, N, K, 1, s, sc);
}
// Per-tap gather implicit GEMM: forward (src = x, wk = w) or stride-1 input gradient (DGRAD: src = dy, wk = wt).
template <bool DGRAD, class EPI>
static void launch_conv_gemm(const float* src, const float* wk, const ConvGeom& g, const EPI& e, ConvTile tile, int M, int N, int K, int kid,
                             void* ws, long ws_bytes, hipStream_t s) {
    with_tile(tile, [&](auto bm, auto bn) {
        constexpr int BM = decltype(bm)::value, BN = decltype(bn)::value;
        ConvGatherKC<BM, DGRAD> al{src, g, M};
        DenseKC<BN, true> bl{wk, (long)K, N};
        launch_tailsplit_or_plain<ConvGatherKC<BM, DGRAD>, DenseKC<BN, true>, EPI, BM, BN>(al, bl, e, M, N, K, kid, ws, ws_bytes, s);
    });
}
// Position-major rows: border pixels skip their out-of-bounds taps (mfma_gemm.h, ConvGatherPM).  C = channels of src.
template <bool DGRAD, class EPI>
static void launch_conv_pm(const float* src, const float* wk, const ConvGeom& g, const EPI& e, int M, int N, int K, int C, int kid, hipStream_t s) {
    ConvGatherPM<64, DGRAD> al{src, g, M, 0ull};
    DenseKCTapList<64> bl{wk, (long)K, N, C, 0ull};
    SplitCtl sc{nullptr, nullptr, nullptr, sbl_next_stamp_slot(kid)};
    const dim3 grid(sbl_cdiv(N, 64), sbl_cdiv(M, 64), 1);
    sbl_note_route(3, sbl_route_tile(64, 64), 0, 0);
    sbl_with_prec([&](auto p) {
        hipLaunchKernelGGL((sbl_conv_pm_kernel<ConvGatherPM<64, DGRAD>, DenseKCTapList<64>, EPI, 64, 64, DGRAD, decltype(p)::value>), grid, dim3(256), 0, s,
                           al, bl, e, sc, M, N);
    });
}

extern "C" int sbl_conv2d_fwd(const float* x, const float* w, float* y, double* stats, int stats_zeroed, int NIMG, int H, int W,
                              int Cin, int Cout, int KH, int KW, int stride, int pad, void* ws, long ws_bytes, sbl_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int e = check_conv("sbl_conv2d_fwd", NIMG, H, W, Cin, Cout, KH, KW, stride, pad)) return e;
    SBL_REQUIRE(x && w && y && sbl_aligned16(x) && sbl_aligned16(w), "sbl_conv2d_fwd: null/unaligned pointer");
    const int Ho = out_dim(H, KH, stride, pad), Wo = out_dim(W, KW, stride, pad);
    const int M = NIMG * Ho * Wo, N = Cout, K = KH * KW * Cin;
    ConvGeom g{NIMG, Ho, Wo, H, W, Cin, KH, KW, stride, pad, 0, 0, 0, 0, {0, 0, 0, 0}, {0, 0, 0, 0}};
    sbl_geom_finish(g);
    if (stats && !stats_zeroed) SBL_HIP(hipMemsetAsync(stats, 0, sizeof(double) * 2 * Cout, s));
    SBL_REQUIRE(!ws || (sbl_aligned16(ws) && ws_bytes >= (long)sizeof(int) * kConvWsCounters), "sbl_conv2d_fwd: workspace unaligned or < 16 KiB");
    if (KH == 3 && stride == 1) {
        // every map sbl_conv_patch_tile accepts in the current mode (layers 1 and 2 in all split-bf16 modes, layers 3 and 4 too
        // at two planes / one plane): the input patch of a tile staged once in LDS for all nine taps (conv_patch.h)
        bool done;
        const PatchEpi pe{y, stats, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        if (stats) done = sbl_launch_conv_patch<false, 1>(x, w, pe, NIMG, H, W, Cin, Cout, SBL_KID_CONV_FWD, s);
        else done = sbl_launch_conv_patch<false, 0>(x, w, pe, NIMG, H, W, Cin, Cout, SBL_KID_CONV_FWD, s);
        if (done) {
            SBL_LAUNCH_CHECK("sbl_conv2d_fwd(patch)");
            return 0;
        }
    }
    if (conv_pm_ok(Ho, Wo, KH, stride)) {
        with_fwd_epi(y, N, stats, rows_pm(NIMG, Ho * Wo), [&](const auto& e) { launch_conv_pm<false>(x, w, g, e, M, N, K, Cin, SBL_KID_CONV_FWD, s); });
        SBL_LAUNCH_CHECK("sbl_conv2d_fwd(pm)");
        return 0;
    }
    const ConvTile tile = conv_tile(N, (long)sbl_cdiv(M, 128) * sbl_cdiv(N, 128), (long)sbl_cdiv(M, 128) * sbl_cdiv(N, 64), true, false);
    with_fwd_epi(y, N, stats, kRowsDirect, [&](const auto& e) { launch_conv_gemm<false>(x, w, g, e, tile, M, N, K, SBL_KID_CONV_FWD, ws, ws_bytes, s); });
    SBL_LAUNCH_CHECK("sbl_conv2d_fwd");
    return 0;
}

// One parity class of a stride-2 input gradient: its geometry, the linear indices of its taps, GEMM rows and depth.
struct DgradClass { ConvGeom g; int lin[4]; int M, K, ph, pw; };
static int conv2d_dgrad_impl(const float* dy, const float* wt, float* dx, int NIMG, int H, int W, int Cin, int Cout,
                             int KH, int KW, int stride, int pad, void* ws, long ws_bytes, sbl_stream_t stream,
                             const DgradFuse& f, int compact_out) {
    hipStream_t s = (hipStream_t)stream;
    if (int e = check_conv("sbl_conv2d_dgrad", NIMG, H, W, Cin, Cout, KH, KW, stride, pad)) return e;
    SBL_REQUIRE(dy && wt && dx && sbl_aligned16(dy) && sbl_aligned16(wt), "sbl_conv2d_dgrad: null/unaligned pointer");
    const int Ho = out_dim(H, KH, stride, pad), Wo = out_dim(W, KW, stride, pad);
    const bool fused = f.addend || f.sums;
    if (f.sums) {
        SBL_REQUIRE(f.y && f.x && f.mean && f.inv && (!f.x2 || (f.mean2 && f.inv2)), "sbl_conv2d_dgrad_fused: incomplete BatchNorm operands");
        if (!f.sums_zeroed) SBL_HIP(hipMemsetAsync(f.sums, 0, sizeof(double) * (f.x2 ? 4 : 2) * Cin, s));
    }
    SBL_REQUIRE(!f.addend || f.add_class00 == (stride == 2), "sbl_conv2d_dgrad_fused: the compact addend belongs to stride-2 convolutions (and only to them)");
    SBL_REQUIRE(!compact_out || (KH == 1 && stride == 2 && !fused), "sbl_conv2d_dgrad: compact output is the 1x1 / stride-2 case");
    if (stride == 2) {
        // Input pixel (ih, iw) only receives taps with kh = ih + pad (mod 2), kw likewise: 1 + 2 + 2 + 4 of the 9 taps
        // over the four parity classes (3x3), or the even/even class alone (1x1).  One dense implicit GEMM per class
        // (rows = the class's pixels, k = its taps) does 1/4 of the work of gathering zeros for the other taps.
        const int N = Cin;
        if (KH == 1 && !compact_out) SBL_HIP(hipMemsetAsync(dx, 0, sizeof(float) * (size_t)NIMG * H * W * Cin, s));
        // the classes, heaviest (most taps) first
        DgradClass cls[4];
        int nc = 0;
        for (int ph = 0; ph < 2; ++ph)
            for (int pw = 0; pw < 2; ++pw) {
                DgradClass c{ConvGeom{NIMG, (H - ph + 1) / 2, (W - pw + 1) / 2, Ho, Wo, Cout, KH, KW, stride, pad, 1, ph, pw, 0, {0, 0, 0, 0}, {0, 0, 0, 0}}, {0, 0, 0, 0}, 0, 0, ph, pw};
                sbl_geom_finish(c.g);
                for (int kh = 0; kh < KH; ++kh)
                    for (int kw = 0; kw < KW; ++kw)
                        if (((ph + pad - kh) & 1) == 0 && ((pw + pad - kw) & 1) == 0) {
                            c.g.tkh[c.g.ntaps] = kh; c.g.tkw[c.g.ntaps] = kw; c.lin[c.g.ntaps] = kh * KW + kw;
                            ++c.g.ntaps;
                        }
                c.M = NIMG * c.g.OH * c.g.OW;
                c.K = c.g.ntaps * Cout;
                if (c.g.ntaps == 0 || c.M == 0) continue;
                int at = nc++;
                while (at > 0 && cls[at - 1].K < c.K) { cls[at] = cls[at - 1]; --at; }
                cls[at] = c;
            }
        if (nc == 0) return 0;
        SplitCtl sc{nullptr, nullptr, nullptr, sbl_next_stamp_slot(SBL_KID_CONV_DGRAD)};
        const int cmap = compact_out ? 0 : 1;
        long t128 = 0, t128x64 = 0;
        for (int i = 0; i < nc; ++i) {
            t128 += (long)sbl_cdiv(cls[i].M, 128) * sbl_cdiv(N, 128);
            t128x64 += (long)sbl_cdiv(cls[i].M, 128) * sbl_cdiv(N, 64);
        }
        const ConvTile tile = conv_tile(N, t128, t128x64, false, f.sums != nullptr);
        // the classes' tile ranges inside the one grid
        int t0[SBL_MAX_CLASSES + 1];
        long tt = 0;
        for (int i = 0; i <= SBL_MAX_CLASSES; ++i) {
            t0[i] = (int)tt;
            if (i < nc) tt += (long)sbl_cdiv(cls[i].M, conv_tile_m(tile)) * sbl_cdiv(N, conv_tile_n(tile));
        }
        SBL_REQUIRE(tt < (1L << 30), "sbl_conv2d_dgrad: too many tiles");
        with_dgrad_epi(dx, N, f, [&](auto make) {
            with_tile(tile, [&](auto bm, auto bn) {
                constexpr int BM = decltype(bm)::value, BN = decltype(bn)::value;
                using AL = ConvGatherKC<BM, true>;
                using BL = DenseKCTaps<BN>;
                using EPI = decltype(make(kRowsDirect, f.addend, 0L));
                ClassSet<AL, BL, EPI> cs;
                cs.nclass = nc;
                cs.tiles_n = sbl_cdiv(N, BN);
                for (int i = 0; i < SBL_MAX_CLASSES; ++i) {
                    const DgradClass& c = cls[i < nc ? i : 0];
                    const float* add = (f.addend && c.ph == 0 && c.pw == 0) ? f.addend : nullptr;
                    cs.al[i] = AL{dy, c.g, c.M};
                    cs.bl[i] = BL{wt, (long)KH * KW * Cout, N, Cout, {c.lin[0], c.lin[1], c.lin[2], c.lin[3]}};
                    cs.epi[i] = make(RowMap{cmap, c.g.OH, c.g.OW, H, W, c.ph, c.pw}, add, (long)N);
                    cs.M[i] = c.M; cs.K[i] = c.K; cs.t0[i] = t0[i];
                }
                cs.t0[SBL_MAX_CLASSES] = t0[SBL_MAX_CLASSES];
                sbl_note_route(5, sbl_route_tile(BM, BN), 0, 0);
                sbl_with_prec([&](auto p) {
                    hipLaunchKernelGGL((sbl_conv_classes_kernel<AL, BL, EPI, BM, BN, decltype(p)::value>), dim3((unsigned)tt), dim3(256), 0, s, cs, sc, N);
                });
            });
        });
        SBL_LAUNCH_CHECK("sbl_conv2d_dgrad(classes)");
        return 0;
    }
    const int M = NIMG * H * W, N = Cin, K = KH * KW * Cout;
    ConvGeom g{NIMG, H, W, Ho, Wo, Cout, KH, KW, stride, pad, 0, 0, 0, 0, {0, 0, 0, 0}, {0, 0, 0, 0}};
    sbl_geom_finish(g);
    SBL_REQUIRE(!ws || (sbl_aligned16(ws) && ws_bytes >= (long)sizeof(int) * kConvWsCounters), "sbl_conv2d_dgrad: workspace unaligned or < 16 KiB");
    if (KH == 3 && stride == 1) {
        // the maps sbl_conv_patch_tile accepts (see sbl_conv2d_fwd): patch-resident kernel with mirrored taps (conv_patch.h)
        bool done;
        const PatchEpi pe{dx, f.sums, f.addend, f.y, f.x, f.mean, f.inv, f.x2, f.mean2, f.inv2};
        if (f.sums) done = sbl_launch_conv_patch<true, 2>(dy, wt, pe, NIMG, H, W, Cout, Cin, SBL_KID_CONV_DGRAD, s);
        else if (f.addend) done = sbl_launch_conv_patch<true, 3>(dy, wt, pe, NIMG, H, W, Cout, Cin, SBL_KID_CONV_DGRAD, s);
        else done = sbl_launch_conv_patch<true, 0>(dy, wt, pe, NIMG, H, W, Cout, Cin, SBL_KID_CONV_DGRAD, s);
        if (done) {
            SBL_LAUNCH_CHECK("sbl_conv2d_dgrad(patch)");
            return 0;
        }
    }
    if (conv_pm_ok(H, W, KH, stride)) {
        with_dgrad_epi(dx, N, f, [&](auto make) {
            launch_conv_pm<true>(dy, wt, g, make(rows_pm(NIMG, H * W), f.addend, 0L), M, N, K, Cout, SBL_KID_CONV_DGRAD, s);
        });
        SBL_LAUNCH_CHECK("sbl_conv2d_dgrad(pm)");
        return 0;
    }
    const ConvTile tile = conv_tile(N, (long)sbl_cdiv(M, 128) * sbl_cdiv(N, 128), (long)sbl_cdiv(M, 128) * sbl_cdiv(N, 64), true, f.sums != nullptr);
    with_dgrad_epi(dx, N, f, [&](auto make) {
        launch_conv_gemm<true>(dy, wt, g, make(kRowsDirect, f.addend, 0L), tile, M, N, K, SBL_KID_CONV_DGRAD, ws, ws_bytes, s);
    });
    SBL_LAUNCH_CHECK("sbl_conv2d_dgrad");
    return 0;
}
static const DgradFuse kNoFuse{nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
extern "C" int sbl_conv2d_dgrad(const float* dy, const float* wt, float* dx, int NIMG, int H, int W, int Cin, int Cout,
                                int KH, int KW, int stride, int pad, void* ws, long ws_bytes, sbl_stream_t stream) {
    return conv2d_dgrad_impl(dy, wt, dx, NIMG, H, W, Cin, Cout, KH, KW, stride, pad, ws, ws_bytes, stream, kNoFuse, 0);
}
extern "C" int sbl_conv2d_dgrad_bnstats(const float* dy, const float* wt, float* dx, int NIMG, int H, int W, int Cin, int Cout,
                                        int KH, int KW, int stride, int pad, void* ws, long ws_bytes, const float* act,
                                        const float* pre, const float* mean, const float* invstd, double* sums,
                                        int sums_zeroed, sbl_stream_t stream) {
    SBL_REQUIRE(act && pre && mean && invstd && sums, "sbl_conv2d_dgrad_bnstats: null statistics operand");
    return conv2d_dgrad_impl(dy, wt, dx, NIMG, H, W, Cin, Cout, KH, KW, stride, pad, ws, ws_bytes, stream,
                             DgradFuse{nullptr, 0, act, pre, mean, invstd, nullptr, nullptr, nullptr, sums, sums_zeroed}, 0);
}
extern "C" int sbl_conv2d_dgrad_fused(const float* dy, const float* wt, float* dx, int NIMG, int H, int W, int Cin, int Cout,
                                      int KH, int KW, int stride, int pad, void* ws, long ws_bytes, const float* addend,
                                      const float* act, const float* pre, const float* mean, const float* invstd,
                                      const float* pre2, const float* mean2, const float* invstd2, double* sums,
                                      int sums_zeroed, sbl_stream_t stream) {
    return conv2d_dgrad_impl(dy, wt, dx, NIMG, H, W, Cin, Cout, KH, KW, stride, pad, ws, ws_bytes, stream,
                             DgradFuse{addend, addend && stride == 2, act, pre, mean, invstd, pre2, mean2, invstd2, sums, sums_zeroed}, 0);
}
extern "C" int sbl_conv1x1s2_dgrad_compact(const float* dy, const float* wt, float* dx_compact, int NIMG, int H, int W, int Cin,
                                           int Cout, void* ws, long ws_bytes, sbl_stream_t stream) {
    return conv2d_dgrad_impl(dy, wt, dx_compact, NIMG, H, W, Cin, Cout, 1, 1, 2, 0, ws, ws_bytes, stream, kNoFuse, 1);
}

// K splits of a weight-gradient launch: about `target` workgroups over `tiles` output tiles, chunks of at least 256 pixels
static inline int wgrad_splits(long target, long tiles, int K) {
    int splits = (int)((target + tiles - 1) / tiles);
    if (splits > K / 256) splits = K / 256;
    return splits < 1 ? 1 : splits;
}
extern "C" int sbl_conv2d_wgrad(const float* x, const float* dy, float* dw, int NIMG, int H, int W, int Cin, int Cout,
                                int KH, int KW, int stride, int pad, int dw_zeroed, sbl_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int e = check_conv("sbl_conv2d_wgrad", NIMG, H, W, Cin, Cout, KH, KW, stride, pad)) return e;
    SBL_REQUIRE(x && dy && dw && sbl_aligned16(x) && sbl_aligned16(dy), "sbl_conv2d_wgrad: null/unaligned pointer");
    const int Ho = out_dim(H, KH, stride, pad), Wo = out_dim(W, KW, stride, pad);
    const int M = Cout, N = KH * KW * Cin, K = NIMG * Ho * Wo;   // reduce over output pixels
    ConvGeom g{NIMG, Ho, Wo, H, W, Cin, KH, KW, stride, pad, 0, 0, 0, 0, {0, 0, 0, 0}, {0, 0, 0, 0}};
    sbl_geom_finish(g);
    if (!dw_zeroed) SBL_HIP(hipMemsetAsync(dw, 0, sizeof(float) * (size_t)M * N, s));
    // split the pixel reduction: 128x128 tiles for the 128+-channel layers (twice the flops per staged byte), 64x64
    // otherwise, and 6 / 12 workgroups per CU so that the uneven last chunks and the atomic epilogues of one
    // workgroup hide behind the others (measured, tools/bench_conv.py: 465/477/511/515 us -> 411/355/437/453 us for
    // layers 1-4); chunks stay >= 256 pixels
    const bool big = M >= 128 && N >= 1152 && !(stride == 2 && sbl_wg_s2_small);
    const int wg_target = stride == 2 ? sbl_wg_s2_target : (big ? 1536 : 3072);
    // (the stamp slot is taken before the patch-resident route is tried: whichever route launches uses it)
    SplitCtl sc{nullptr, nullptr, nullptr, sbl_next_stamp_slot(SBL_KID_CONV_WGRAD)};
    if (KH == 3 && KW == 3 && stride == 1 && pad == 1 && sbl_launch_conv_patch_wgrad(x, dy, dw, NIMG, H, W, Cin, Cout, sc.stamp, s)) {
        SBL_LAUNCH_CHECK("sbl_conv2d_wgrad(patch)");
        return 0;
    }
    const EpiStore<2, false> e{dw, (long)N, nullptr, 0, nullptr, nullptr, 0};
    if (conv_pm_ok(Ho, Wo, KH, stride) && big && M >= 128 && Cin % 128 == 0) {
        // one tap per tile of the (tap, ci) axis: contract only over the pixels that tap can reach
        auto pm = [&](auto t) {
            constexpr int T = decltype(t)::value;
            const int splits = wgrad_splits(T == 128 ? wg_target : 2 * wg_target, (long)sbl_cdiv(M, T) * sbl_cdiv(N, T), K);
            DenseMCPM<T> al{dy, (long)Cout, M, NIMG, Ho, Wo, g.fdNIMG, PmRect{0, 0, 1, 0, 0, 1.f}};
            ConvGatherMCPM<T> bl{x, g, N, PmRect{0, 0, 1, 0, 0, 1.f}};
            sbl_note_route(7, sbl_route_tile(T, T), 0, 0);
            sbl_with_prec([&](auto p) {
                hipLaunchKernelGGL((sbl_conv_pm_wgrad_kernel<DenseMCPM<T>, ConvGatherMCPM<T>, EpiStore<2, false>, T, T, decltype(p)::value>),
                                   dim3(sbl_cdiv(M, T), sbl_cdiv(N, T), splits), dim3(256), 0, s, al, bl, e, sc, M, N);
            });
        };
        if (M <= sbl_pm_wg64_max_m) pm(sbl_int<64>{});
        else pm(sbl_int<128>{});
        SBL_LAUNCH_CHECK("sbl_conv2d_wgrad(pm)");
        return 0;
    }
    auto plain = [&](auto t) {
        constexpr int T = decltype(t)::value;
        DenseMC<T, true> al{dy, (long)Cout, M};
        ConvGatherMC<T> bl{x, g, N};
        sbl_note_route(8, sbl_route_tile(T, T), 0, 0);
        sbl_launch_gemm<DenseMC<T, true>, ConvGatherMC<T>, EpiStore<2, false>, T, T>(al, bl, e, M, N, K, wgrad_splits(wg_target, (long)sbl_cdiv(M, T) * sbl_cdiv(N, T), K), s, sc);
    };
    if (big && M >= 128) plain(sbl_int<128>{});
    else plain(sbl_int<64>{});
    SBL_LAUNCH_CHECK("sbl_conv2d_wgrad");
    return 0;
}

// ------------------------------------------------------------------ weight layout
// OIHW (state-dict layout) -> OHWI [Cout][KH][KW][Cin]  (+ dgrad operand [Cin][KH][KW][Cout])
__global__ void weight_pack_kernel(const float* __restrict__ w, float* __restrict__ ohwi, float* __restrict__ wt,
                                   int Cout, int Cin, int KH, int KW, double* __restrict__ zero, int nzero) {
    long n = (long)Cout * Cin * KH * KW;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nzero; i += gridDim.x * blockDim.x) zero[i] = 0.0;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        // i indexes OHWI
        int ci = i % Cin;
        long t = i / Cin;
        int kw = t % KW;
        t /= KW;
        int kh = t % KH;
        int co = t / KH;
        float v = w[(((long)co * Cin + ci) * KH + kh) * KW + kw];
        ohwi[i] = v;
        if (wt) wt[(((long)ci * KH + kh) * KW + kw) * Cout + co] = v;
    }
}
__global__ void wgrad_unpack_kernel(const float* __restrict__ ohwi, float* __restrict__ oihw, int Cout, int Cin, int KH,
                                    int KW, int accumulate) {
    long n = (long)Cout * Cin * KH * KW;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        // i indexes OIHW
        int kw = i % KW;
        long t = i / KW;
        int kh = t % KH;
        t /= KH;
        int ci = t % Cin;
        int co = t / Cin;
        const float g = ohwi[(((long)co * KH + kh) * KW + kw) * Cin + ci];
        oihw[i] = accumulate ? oihw[i] + g : g;
    }
}
extern "C" int sbl_conv_weight_pack(const float* w, float* ohwi, float* wt, int Cout, int Cin, int KH, int KW,
                                    double* zero, int nzero, sbl_stream_t stream) {
    SBL_REQUIRE(w && ohwi && Cout > 0 && Cin > 0 && KH > 0 && KW > 0 && nzero >= 0 && (zero || !nzero), "sbl_conv_weight_pack: bad args");
    long n = (long)Cout * Cin * KH * KW;
    hipLaunchKernelGGL(weight_pack_kernel, dim3(sbl_cdiv(n, 256) > 2048 ? 2048 : sbl_cdiv(n, 256)), dim3(256), 0,
                       (hipStream_t)stream, w, ohwi, wt, Cout, Cin, KH, KW, zero, nzero);
    SBL_LAUNCH_CHECK("sbl_conv_weight_pack");
    return 0;
}
extern "C" int sbl_conv_wgrad_unpack(const float* ohwi, float* oihw, int Cout, int Cin, int KH, int KW, int accumulate,
                                     sbl_stream_t stream) {
    SBL_REQUIRE(ohwi && oihw && Cout > 0 && Cin > 0 && KH > 0 && KW > 0, "sbl_conv_wgrad_unpack: bad args");
    long n = (long)Cout * Cin * KH * KW;
    hipLaunchKernelGGL(wgrad_unpack_kernel, dim3(sbl_cdiv(n, 256) > 2048 ? 2048 : sbl_cdiv(n, 256)), dim3(256), 0,
                       (hipStream_t)stream, ohwi, oihw, Cout, Cin, KH, KW, accumulate);
    SBL_LAUNCH_CHECK("sbl_conv_wgrad_unpack");
    return 0;
}

// ------------------------------------------------------------------ global average pool (NHWC)
__global__ void avgpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int NIMG, int HW, int C) {
    long n = (long)NIMG * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int c = i % C;
        long img = i / C;
        float s = 0.f;
        for (int p = 0; p < HW; ++p) s += x[(img * HW + p) * C + c];
        y[i] = s / (float)HW;
    }
}
__global__ void avgpool_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int NIMG, int HW, int C) {
    long n = (long)NIMG * HW * C;
    const float inv = 1.f / (float)HW;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        int c = i % C;
        long img = i / ((long)HW * C);
        dx[i] = dy[img * C + c] * inv;
    }
}
extern "C" int sbl_avgpool_fwd(const float* x, float* y, int NIMG, int HW, int C, sbl_stream_t stream) {
    SBL_REQUIRE(x && y && NIMG > 0 && HW > 0 && C > 0, "sbl_avgpool_fwd: bad args");
    long n = (long)NIMG * C;
    hipLaunchKernelGGL(avgpool_fwd_kernel, dim3(sbl_cdiv(n, 256) > 4096 ? 4096 : sbl_cdiv(n, 256)), dim3(256), 0,
                       (hipStream_t)stream, x, y, NIMG, HW, C);
    SBL_LAUNCH_CHECK("sbl_avgpool_fwd");
    return 0;
}
extern "C" int sbl_avgpool_bwd(const float* dy, float* dx, int NIMG, int HW, int C, sbl_stream_t stream) {
    SBL_REQUIRE(dy && dx && NIMG > 0 && HW > 0 && C > 0, "sbl_avgpool_bwd: bad args");
    long n = (long)NIMG * HW * C;
    hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(sbl_cdiv(n, 256) > 4096 ? 4096 : sbl_cdiv(n, 256)), dim3(256), 0,
                       (hipStream_t)stream, dy, dx, NIMG, HW, C);
    SBL_LAUNCH_CHECK("sbl_avgpool_bwd");
    return 0;
}
