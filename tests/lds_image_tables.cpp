// Prints the LDS image layouts of csrc/lds_image.h as tables for tests/test_lds_image_host.py.  Host only: it includes
// that header alone.
//   row <ROW bytes>  |  tr <NV>       the image the following lines belong to
//   w <g> <row> <col>                 writer: linear 16-byte slot g of a 64-row tile -> tile row, first element column
//   r <row> <slot> <off>              reader: byte offset of logical 16-byte slot `slot` of row `row`
//   f <l31> <hh> <s> <off>            row images: read_off of lane (l31, hh), column step s
//   lane <lane> <row> <ch> <sub>      lane geometry of the transposed reads
#include <cstdio>

#include "lds_image.h"

template <class Image, int PER_ROW> static void tables() {
    for (int g = 0; g < 64 * PER_ROW; ++g) {
        const bp::TileSrc s = Image::src(g);
        std::printf("w %d %d %d\n", g, s.row, s.col);
    }
    for (int row = 0; row < 64; ++row)
        for (int slot = 0; slot < PER_ROW; ++slot) std::printf("r %d %d %d\n", row, slot, Image::off(row, slot));
}
template <int ROW> static void row_image() {
    std::printf("row %d\n", ROW);
    tables<bp::RowImage<ROW>, ROW / 16>();
    for (int l31 = 0; l31 < 32; ++l31)
        for (int hh = 0; hh < 2; ++hh)
            for (int s = 0; 2 * s + 1 < ROW / 16; ++s) std::printf("f %d %d %d %d\n", l31, hh, s, bp::RowImage<ROW>::read_off(l31, hh, s));
}
template <int NV> static void tr_image() {
    std::printf("tr %d\n", NV);
    tables<bp::TrImage<NV>, NV * 4>();
}
template <int... ROW> static void row_images() { (row_image<ROW>(), ...); }
template <int... NV> static void tr_images() { (tr_image<NV>(), ...); }

int main() {
    row_images<128, 256, 48, 80, 112, 176, 208, 240>();
    tr_images<1, 2, 3, 4, 5, 8, 10>();
    for (int lane = 0; lane < 64; ++lane) {
        const bp::TrLane t = bp::tr_lane(lane, lane >> 5);
        std::printf("lane %d %d %d %d\n", lane, t.row, t.ch, t.sub);
    }
    return 0;
}
