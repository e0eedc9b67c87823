"""csrc/lds_image.h on the host: the DMA writer's map and the MFMA reader's offsets of every LDS image are one bijection.

tests/lds_image_tables.cpp includes the header alone, is built with g++ and prints, per instantiated image, the writer
table (linear 16-byte slot -> tile row, column) and the reader offsets.  They are compared with the formulas as the
kernels spelled them before the header existed, written out again here; then the properties the layouts exist for are
checked on the printed tables: writer and reader meet, every slot is produced once, the operand reads spread over the banks.
No GPU, no sanitizer, nothing preloaded.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'backpacks-flash-attn_amd', 'csrc')
ROW_PITCHES = [128, 256, 48, 80, 112, 176, 208, 240]   # bytes; the odd slot counts are 2 KD + 1 of flash_fwd_dma.hip
TR_CHUNKS = [1, 2, 3, 4, 5, 8, 10]                     # 64-byte chunks per row
TILE_ROWS = 64


# ---- the layouts, spelled independently of the header ----------------------------------------------------------------------
def row_swz(pitch, row):
    return {128: (row >> 1) & 7, 256: row & 15}.get(pitch, 0)


def tr_swz(nv, row):
    return {2: (row >> 1) & 1, 10: (row >> 1) & 1, 4: row & 3, 8: row & 3}.get(nv, 0)


class RowModel:
    def __init__(self, pitch, swz=row_swz):
        self.pitch, self.per_row, self.swz = pitch, pitch // 16, swz

    def writer(self, g):
        row, stored = divmod(g, self.per_row)
        return row, (stored ^ self.swz(self.pitch, row)) * 8

    def reader(self, row, slot):
        return row * self.pitch + (slot ^ row_swz(self.pitch, row)) * 16


class TrModel:
    def __init__(self, nv, swz=tr_swz):
        self.nv, self.per_row, self.swz = nv, nv * 4, swz

    def writer(self, c):
        row, stored = divmod(c, self.per_row)
        c64 = (stored >> 2) ^ self.swz(self.nv, row)
        return row, ((c64 << 2) | (stored & 3)) * 8

    def reader(self, row, ch):
        c64 = (ch >> 2) ^ tr_swz(self.nv, row)
        return row * self.nv * 64 + ((c64 << 2) | (ch & 3)) * 16


def round_trip_ok(writer, reader, per_row):
    """writer then reader returns to the linear slot, and the reader's offsets cover the image exactly once"""
    n = TILE_ROWS * per_row
    for g in range(n):
        row, col = writer(g)
        if col % 8 or not 0 <= col // 8 < per_row or reader(row, col // 8) != 16 * g:
            return False
    offs = sorted(reader(row, slot) for row in range(TILE_ROWS) for slot in range(per_row))
    return offs == [16 * i for i in range(n)]


# ---- the header's tables --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tables(tmp_path_factory):
    cxx = shutil.which('g++')
    assert cxx, 'g++ not found'
    exe = str(tmp_path_factory.mktemp('lds_image') / 'lds_image_tables')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, os.path.join(ROOT, 'tests', 'lds_image_tables.cpp'),
                    '-o', exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    images, lanes, cur = {}, {}, None
    for line in out.splitlines():
        f = line.split()
        if f[0] in ('row', 'tr'):
            cur = images[(f[0], int(f[1]))] = {'w': {}, 'r': {}, 'f': {}}
        elif f[0] == 'lane':
            lanes[int(f[1])] = tuple(int(x) for x in f[2:])
        else:
            v = [int(x) for x in f[1:]]
            cur[f[0]][tuple(v[:-2]) if f[0] == 'w' else tuple(v[:-1])] = tuple(v[-2:]) if f[0] == 'w' else v[-1]
    return images, lanes


def models():
    return [(('row', p), RowModel(p)) for p in ROW_PITCHES] + [(('tr', nv), TrModel(nv)) for nv in TR_CHUNKS]


def test_every_instantiated_image_is_printed(tables):
    images, lanes = tables
    assert sorted(images) == sorted(key for key, _ in models())
    assert sorted(lanes) == list(range(64))


@pytest.mark.parametrize('key,model', models(), ids=lambda x: '%s%d' % x if isinstance(x, tuple) else '')
def test_tables_match_the_formulas_the_kernels_spelled(tables, key, model):
    img = tables[0][key]
    n = TILE_ROWS * model.per_row
    assert img['w'] == {(g,): model.writer(g) for g in range(n)}
    assert img['r'] == {(row, slot): model.reader(row, slot) for row in range(TILE_ROWS) for slot in range(model.per_row)}
    if key[0] == 'row':   # the reader's lane form: row l31, logical slot 2 s + hh
        steps = (model.per_row - (model.per_row & 1)) // 2
        assert img['f'] == {(l31, hh, s): model.reader(l31, 2 * s + hh)
                            for l31 in range(32) for hh in range(2) for s in range(steps)}


@pytest.mark.parametrize('key,model', models(), ids=lambda x: '%s%d' % x if isinstance(x, tuple) else '')
def test_writer_and_reader_meet_and_every_slot_is_produced_once(tables, key, model):
    img = tables[0][key]
    assert round_trip_ok(lambda g: img['w'][(g,)], lambda row, slot: img['r'][(row, slot)], model.per_row)


@pytest.mark.parametrize('pitch', ROW_PITCHES)
def test_row_image_b128_reads_touch_every_bank_once(tables, pitch):
    """16 consecutive rows from a multiple of 16, one logical slot: 16 distinct 16-byte positions modulo 256 bytes"""
    img = tables[0][('row', pitch)]
    for base in range(0, TILE_ROWS, 16):
        for slot in range(pitch // 16):
            pos = {img['r'][(base + i, slot)] % 256 // 16 for i in range(16)}
            assert len(pos) == 16, (pitch, base, slot)


@pytest.mark.parametrize('nv', TR_CHUNKS)
def test_transposed_reads_spread_over_the_four_bank_quarters(tables, nv):
    """rows 4 m .. 4 m + 3 at one logical 64-byte chunk lie in four different 64-byte quarters of a 256-byte bank line"""
    img = tables[0][('tr', nv)]
    for m in range(TILE_ROWS // 4):
        for c64 in range(nv):
            quarters = {img['r'][(4 * m + i, 4 * c64)] % 256 // 64 for i in range(4)}
            assert len(quarters) == 4, (nv, m, c64)


def test_lane_geometry_of_the_transposed_read(tables):
    lanes = tables[1]
    for lane in range(64):
        hh = lane >> 5
        assert lanes[lane] == (4 * hh + ((lane & 15) >> 2), ((lane >> 4) & 1) * 2 + ((lane & 3) >> 1), (lane & 1) * 8)


def test_a_wrong_swizzle_fails_the_round_trip():
    """the check can fail: a writer that swizzles with other row bits than the reader does not return to its slot"""
    for good, bad in ((RowModel(128), RowModel(128, swz=lambda pitch, row: row & 7)),
                      (RowModel(256), RowModel(256, swz=lambda pitch, row: (row >> 1) & 15)),
                      (TrModel(2), TrModel(2, swz=lambda nv, row: row & 1)),
                      (TrModel(10), TrModel(10, swz=lambda nv, row: 0)),
                      (TrModel(8), TrModel(8, swz=lambda nv, row: (row >> 1) & 3))):
        assert round_trip_ok(good.writer, good.reader, good.per_row)
        assert not round_trip_ok(bad.writer, bad.reader, bad.per_row)
