// LDS tile images: one definition of where the DMA writer puts a tile's 16-byte slots and where the MFMA reads find them.
// The DMA writes LDS linearly (lane i of 1-KiB piece p lands at byte p * 1024 + i * 16, bp_dma.h), so the XOR swizzles that
// keep the operand reads free of bank conflicts sit on its SOURCE side: a lane fetches the (row, column) the reader will
// look for at that byte.  Where writer and reader disagree nothing faults, a kernel multiplies the wrong columns: each
// image defines the bijection once (`off`), derives the writer (`src`) from it, and a static_assert proves that they meet.
// Plain constexpr integer functions, no HIP header: a host compiler includes this file alone (tests/test_lds_image_host.py).
#pragma once
namespace bp {
#define BP_IMG constexpr __attribute__((always_inline)) inline

struct TileSrc { int row, col; };   // what a lane fetches: tile row, first 16-bit element column

// Row image: rows of ROW bytes in 16-byte slots, read with ds_read_b128 by 32 lanes at 32 consecutive rows and one logical
// slot.  A pitch of 128 / 256 B XOR-swizzles the slots so that such a read touches every bank once (only row bits 0..3
// enter: +32 rows keep a lane's swizzle); an ODD slot count needs none, (row * SLOTS + slot) mod 16 is distinct over 16 rows.
template <int ROW> struct RowImage {
    static constexpr int SLOTS = ROW / 16;
    static_assert(ROW == 128 || ROW == 256 || (ROW % 16 == 0 && SLOTS % 2 == 1), "pitch: 128, 256 or an odd slot count");
    static BP_IMG int swz(int row) { return ROW == 128 ? ((row >> 1) & 7) : ROW == 256 ? (row & 15) : 0; }
    static BP_IMG int off(int row, int slot) { return row * ROW + ((slot ^ swz(row)) * 16); }   // byte of logical slot
    static BP_IMG int read_off(int l31, int hh, int s) { return off(l31, 2 * s + hh); }        // lane's fragment of column step s
    static BP_IMG TileSrc src(int g) {   // writer: linear slot g of the image (the XOR is an involution: stored -> logical)
        const int row = g / SLOTS;
        return TileSrc{row, ((g - row * SLOTS) ^ swz(row)) * 8};
    }
};
// Transposed-read image: rows of NV 64-byte chunks, read with ds_read_b64_tr_b16, which serves 32 lanes = 4 consecutive
// rows x 64 B at once; the XOR on the chunk index puts those 4 segments in the 4 quarters of the 64 banks.  NV odd: distinct
// by construction;  NV = 2, 10: rows r and r + 2 would collide;  NV = 4, 8: all four would.  (+8 rows keep the swizzle.)
template <int NV> struct TrImage {
    static constexpr int ROW = NV * 64, CH = NV * 4;   // bytes, 16-byte chunks per row
    static BP_IMG int flip(int row, int ch) {   // logical 16-byte chunk <-> stored one
        int c64 = ch >> 2;
        if (NV % 4 == 0) c64 ^= row & 3;
        else if (NV % 2 == 0) c64 ^= (row >> 1) & 1;
        return (c64 << 2) | (ch & 3);
    }
    static BP_IMG int off(int row, int ch) { return row * ROW + flip(row, ch) * 16; }   // byte of logical chunk
    static BP_IMG TileSrc src(int c) { return TileSrc{c / CH, flip(c / CH, c - c / CH * CH) * 8}; }   // writer: linear chunk c
};
template <int NV> BP_IMG int v_lds_off(int row, int ch) { return TrImage<NV>::off(row, ch); }
template <int ROW> BP_IMG int k_swz(int row) { return RowImage<ROW>::swz(row); }

// Where a lane points ds_read_b64_tr_b16 to receive, for its column of a 32-column block, the keys its P^T registers hold
// (bp_common.h): row within 16 keys (+8: second read), 16-byte chunk of the block's four, byte in the chunk.  hh = lane >> 5.
struct TrLane { int row, ch, sub; };
BP_IMG TrLane tr_lane(int lane, int hh) {
    return TrLane{4 * hh + ((lane & 15) >> 2), ((lane >> 4) & 1) * 2 + ((lane & 3) >> 1), (lane & 1) * 8};
}

// Over a 64-row tile: the writer's (row, column) of slot g is read back at byte 16 g, and every slot is produced exactly once.
template <class Image, int PER_ROW> constexpr bool lds_image_ok() {
    bool seen[64 * PER_ROW] = {};
    for (int g = 0; g < 64 * PER_ROW; ++g)
        if (Image::src(g).col % 8 != 0 || Image::off(Image::src(g).row, Image::src(g).col / 8) != g * 16) return false;
    for (int i = 0; i < 64 * PER_ROW; ++i) {
        const int o = Image::off(i / PER_ROW, i % PER_ROW);
        if (o < 0 || o % 16 != 0 || o / 16 >= 64 * PER_ROW || seen[o / 16]) return false;
        seen[o / 16] = true;
    }
    return true;
}
template <int... ROW> constexpr bool row_images_ok() { return (lds_image_ok<RowImage<ROW>, ROW / 16>() && ...); }
template <int... NV> constexpr bool tr_images_ok() { return (lds_image_ok<TrImage<NV>, NV * 4>() && ...); }
static_assert(row_images_ok<128, 256, 48, 80, 112, 176, 208, 240>(), "row image: writer and reader disagree");   // odd: 2 KD + 1 slots
static_assert(tr_images_ok<1, 2, 3, 4, 5, 8, 10>(), "transposed-read image: writer and reader disagree");
}  // namespace bp
