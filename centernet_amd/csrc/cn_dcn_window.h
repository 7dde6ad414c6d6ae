// cn_dcn_window.h -- what the three LDS-window forms of the f32s deformable convolution share:
// cn_dcn2.hip (register-sampling form), cn_dcn3.hip (team form), cn_dcn4.hip (wide form).
//   * the window geometry: an 8 x 16 pixel tile, offsets up to +-3 px inside a 16 x 24 pixel window, the
//     XCD-aware tile order and the tile / window origin (dcnw_tile);
//   * for the team and the wide form, whose windows are filled by LDS-DMA: the swizzled window layout
//     (dcnw_enc), the record regions behind the window, the staging pitch, the zero line, the argument struct;
//   * the host side of a launcher: shape checks, argument fill, launch ladder (which form runs, its blocks and
//     its K split are dcn_route's, cn_dcn.hip).
// A form keeps its step loop, the LDS carve behind the shared regions, its workgroup size and its own checks.
// The prologue (DMA offsets, offset / mask loads, record formation) and the epilogue tail are still written
// out in each kernel: lifted into helpers here they changed the instruction stream of every shipped build.
#pragma once
#include "cn_internal.h"

// one 128-byte line of zeros: the DMA source of window pixels outside the image (one per file that uses it)
inline __device__ __attribute__((aligned(128))) unsigned char dcnw_zero_line[128];

namespace {

// ---- geometry ----------------------------------------------------------------------------------------------
constexpr int DCNW_TX = 16, DCNW_TY = 8, DCNW_PM = DCNW_TX * DCNW_TY;   // tile: 128 output pixels
constexpr int DCNW_RCH = 3;                          // offsets up to +-3 px sample inside the window
constexpr int DCNW_WX = DCNW_TX + 2 + 2 * DCNW_RCH;  // 24
constexpr int DCNW_WY = DCNW_TY + 2 + 2 * DCNW_RCH;  // 16
constexpr int DCNW_WPIX = DCNW_WX * DCNW_WY;         // 384
// DMA-filled window (team, wide): unpadded pixels, swizzled (dcnw_enc); the records sit behind it
constexpr int DCNW_PIXB = 128;                       // bytes per window pixel: 32 plain floats
constexpr int DCNW_ROWB = DCNW_WX * DCNW_PIXB;       // 3072 = 12 x 256: a row starts on bank group 0
constexpr int DCNW_WBYTES = DCNW_WPIX * DCNW_PIXB;   // 49152
constexpr int DCNW_RECW = DCNW_WBYTES;               // float4 [9][128]: corner weights (mask, exponent, validity folded in)
constexpr int DCNW_RECP = DCNW_RECW + 9 * DCNW_PM * 16;   // uint2 [9][128]: swizzled LDS offsets of corners 1 and 2 | far flag + corner
constexpr int DCNW_REC_END = DCNW_RECP + 9 * DCNW_PM * 8; // 76800: a form's own regions start here
constexpr int DCNW_LDC = 68;                         // floats per staged pixel row (64 + 4)
constexpr int DCNW_STG = 32 * DCNW_LDC * 4;          // 8704 bytes of epilogue staging per wave
static_assert(DCNW_ROWB % 256 == 0, "window rows keep the bank-group phase");

typedef _Float16 dcnw_f16x8 __attribute__((ext_vector_type(8)));
typedef float dcnw_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned dcnw_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) char dcnw_lds_char;
typedef __attribute__((address_space(1))) char dcnw_glb_char;
typedef __attribute__((address_space(3))) cn_f32x4 dcnw_lds_f32x4;
typedef __attribute__((address_space(1))) cn_f32x4 dcnw_glb_f32x4;
typedef __attribute__((address_space(3))) dcnw_f16x8 dcnw_lds_f16x8;
typedef __attribute__((address_space(3))) dcnw_u32x2 dcnw_lds_u32x2;
typedef __attribute__((address_space(3))) void dcnw_lds_void;
typedef __attribute__((address_space(1))) const void dcnw_glb_void;

// ---- kernel arguments of the team and the wide form: the common fields, then the per-form extras.
// (cn_dcn2.hip keeps a struct of its own with the same field names -- see there -- so what follows takes the
// argument struct as a template parameter where all three forms use it.)
struct DcnWinArgs {
    const float *x;            // (B, H, W, Cin) plain fp32
    const void *w;             // f32s-packed [tap][cout_pad][cin_pad] row form + the fragment-ordered copy behind it
    const float *bias, *scale, *shift, *om;
    void *y;
    int B, H, W, Cin, Cout, om_pitch, relu;
    int cin_pad, cout_pad, nchunk, tiles_x, tiles_y, out_pitch, out_plain;
    float x_mul;
    uint32_t *range;
    int ksplit;                // K-chunk ranges per tile (blockIdx.z); > 1: raw partial sums
    int dbg;                   // probe build (cn_set_tuning key 9); every form documents its own bits
    float *partial;            // [ksplit][B*H*W][cout_pad] fp32 (splitk_reduce_kernel applies the epilogue)
    int prefetch;              // wide: 1 = L2 prefetch of the weights three steps ahead (cn_set_tuning key 45, default 1)
    int stagger;               // team: start delay of workgroups 256 .. 511 (the second occupant of every CU), units of 256 cycles
    int mask_sigmoid;          // host side only: which build dcnw_launch picks
};

__device__ __forceinline__ void dcnw_barrier()
{
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// swizzled LDS byte offsets of window pixels (wy, wx) and (wy, wx + 1), quad 0 of lane half 0:
// physical 16-byte slot of logical quad q of a pixel = q ^ ((wx >> 1) & 7)
__device__ __forceinline__ unsigned dcnw_enc(int wy, int wx)
{
    const unsigned p = (unsigned)(wy * DCNW_WX + wx);
    const unsigned q1 = p * DCNW_PIXB + ((((unsigned)wx >> 1) & 7u) << 4);
    const unsigned q2 = (p + 1u) * DCNW_PIXB + (((((unsigned)wx + 1u) >> 1) & 7u) << 4);
    return q1 | (q2 << 16);
}

// ---- tile order and origin -----------------------------------------------------------------------------------
struct DcnwTile {
    int b;                     // image
    int ty0, tx0;              // first output pixel of the tile
    int wy0, wx0;              // first input pixel of its window
};

// XCD-aware tile order: contiguous tile ranges per XCD (block b runs on XCD b % 8)
__device__ __forceinline__ DcnwTile dcnw_tile(int tiles_x, int tiles_y)
{
    int bx = blockIdx.x;
    {
        const int q8 = gridDim.x >> 3;
        if (bx < (q8 << 3)) bx = (bx & 7) * q8 + (bx >> 3);
    }
    const int tiles = tiles_x * tiles_y;
    DcnwTile t;
    t.b = bx / tiles;
    const int tr = bx - t.b * tiles;
    t.ty0 = (tr / tiles_x) * DCNW_TY;
    t.tx0 = (tr % tiles_x) * DCNW_TX;
    t.wy0 = t.ty0 - 1 - DCNW_RCH;
    t.wx0 = t.tx0 - 1 - DCNW_RCH;
    return t;
}

// ---- host side of a launcher -------------------------------------------------------------------------------------
// what every window form needs: maps of whole 8 x 16 pixel tiles, whole 32-channel chunks, 16-byte quads in and
// out, 32-bit byte offsets into x
inline bool dcnw_shape_ok(const DcnCall &c)
{
    if ((c.H & 7) || (c.W & 15) || (c.Cin & 31)) return false;
    if ((c.out_pitch & 3) || !cn_aligned16(c.y) || !cn_aligned16(c.x)) return false;
    return (size_t)c.B * c.H * c.W * c.Cin * 4 < ((size_t)1 << 32);
}

// the far path of the records above: 15-bit corner coordinates, 24-bit integer multiplies (pixel index, bytes
// per pixel)
inline bool dcnw_far_ok(const DcnCall &c)
{
    return c.H <= 16383 && c.W <= 16383 && (size_t)c.B * c.H * c.W < ((size_t)1 << 24) && (size_t)c.Cin * 4 < ((size_t)1 << 24);
}

template <class Args = DcnWinArgs>
Args dcnw_fill_args(const DcnCall &c, int ksplit)
{
    Args a = {};
    a.x = c.x; a.w = c.w; a.bias = c.bias; a.scale = c.scale; a.shift = c.shift; a.om = c.om; a.y = c.y;
    a.B = c.B; a.H = c.H; a.W = c.W; a.Cin = c.Cin; a.Cout = c.Cout; a.om_pitch = c.om_pitch;
    a.mask_sigmoid = c.mask_sigmoid; a.relu = c.relu; a.out_pitch = c.out_pitch; a.out_plain = c.out_plain;
    a.cin_pad = c.Cin;
    a.cout_pad = (c.Cout + 31) / 32 * 32;
    a.nchunk = c.Cin / 32;
    a.tiles_x = c.W / DCNW_TX;
    a.tiles_y = c.H / DCNW_TY;
    a.x_mul = c.x_mul; a.range = c.range; a.dbg = c.dbg;
    a.ksplit = ksplit;
    a.partial = ksplit > 1 ? (float *)c.workspace : nullptr;
    return a;
}

// the three builds of a form: probe (key 9 set, sigmoid mask only), sigmoid mask, caller-supplied mask
// (NT threads, LDS bytes of dynamic LDS, grid.y = n_blocks_y blocks of output channels)
template <auto K_DBG, auto K_SIG, auto K_ANY, int NT, int LDS, class Args>
int dcnw_launch(const Args &a, unsigned n_blocks_y, hipStream_t st)
{
    const dim3 grid((unsigned)(a.B * a.tiles_x * a.tiles_y), n_blocks_y, (unsigned)a.ksplit);
    if (a.dbg && a.mask_sigmoid) {
        CN_SET_MAX_LDS_ONCE(K_DBG, LDS);
        hipLaunchKernelGGL(K_DBG, grid, dim3(NT), LDS, st, a);
    } else if (a.mask_sigmoid) {
        CN_SET_MAX_LDS_ONCE(K_SIG, LDS);
        hipLaunchKernelGGL(K_SIG, grid, dim3(NT), LDS, st, a);
    } else {
        CN_SET_MAX_LDS_ONCE(K_ANY, LDS);
        hipLaunchKernelGGL(K_ANY, grid, dim3(NT), LDS, st, a);
    }
    CN_CHECK_LAUNCH();
    return CN_OK;
}

}  // namespace
