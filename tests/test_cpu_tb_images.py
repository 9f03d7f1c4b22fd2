"""CPU-only tests of train.py --tb_images: the numpy model of the grid kernel (ramdsir/tb_images.py grid_model) against answers
derived by hand, the image records of utils/tfevents.py byte for byte and through the reader, the host checksum rd_crc32c against the
RFC 3720 values and the Python routine, and the flag itself."""
import io
import os
import struct
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'ram-dsir_amd'))

from ramdsir import _lib as L, tb_images as T       # noqa: E402
from utils import tfevents as E                      # noqa: E402


# ---------------------------------------------------------------------------------------------------------------- the model
def test_model_two_samples_normalised_grid_by_hand():
    """Samples [[0, 1], [2, 3]] and [[4, 5], [6, 8]]: lo = 0, hi = 8, v = x / 8 (exact), pixel = trunc(255 x / 8):
    0, 31 (31.875), 63 (63.75), 95 (95.625), 127 (127.5), 159 (159.375), 191 (191.25), 255.  The grid is (2 + 4) x (2 (2 + 2) + 2):
    tile 0 at rows 2..3, columns 2..3, tile 1 at columns 6..7, everything else the zero padding; one channel replicated to three."""
    t = np.array([[[[0, 1], [2, 3]]], [[[4, 5], [6, 8]]]], np.float32)
    g = T.grid_model(t, [0, 1], c0=0, nc=1, transform=L.TB_IDENTITY, normalize=True)
    plane = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                      [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                      [0, 0, 0, 31, 0, 0, 127, 159, 0, 0],
                      [0, 0, 63, 95, 0, 0, 191, 255, 0, 0],
                      [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                      [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]], np.uint8)
    assert g.dtype == np.uint8 and g.shape == (6, 10, 3)
    for c in range(3):
        assert np.array_equal(g[:, :, c], plane)


def test_model_single_sample_is_the_image_itself():
    """n == 1: no grid, no padding -- H x W; three channels, not normalised: 0 -> 0, 0.5 -> 127 (127.5), 1 -> 255."""
    t = np.zeros((4, 3, 2, 3), np.float32)
    t[2, 0], t[2, 1], t[2, 2] = 0.0, 0.5, 1.0
    g = T.grid_model(t, [2], c0=0, nc=3, normalize=False)
    assert g.shape == (2, 3, 3)
    assert np.array_equal(g, np.broadcast_to(np.array([0, 127, 255], np.uint8), (2, 3, 3)))
    # normalised: lo = 0, hi = 1: the same picture
    assert np.array_equal(T.grid_model(t, [2], c0=0, nc=3, normalize=True), g)


def test_model_constant_image_divides_by_1e_5():
    """hi == lo: the divisor is 1e-5, x - lo is 0 everywhere: a black grid, no division by zero."""
    t = np.full((2, 1, 2, 2), 0.25, np.float32)
    g = T.grid_model(t, [0, 1], c0=0, nc=1, normalize=True)
    assert g.shape == (6, 10, 3) and not g.any()
    # just above: lo = 0.25, hi - lo = 2^-20 < 1e-5 -> v = 2^-20 / float32(1e-5) = 0.0953..., pixel trunc(24.3) = 24
    t[1, 0, 1, 1] = 0.25 + 2.0 ** -20
    g = T.grid_model(t, [0, 1], c0=0, nc=1, normalize=True)
    assert g[3, 7].tolist() == [24, 24, 24] and int(g.astype(int).sum()) == 72


def test_model_palette_grid_for_labels():
    """Labels 0 / 1 through the palette: class 0 black, class 1 (128, 0, 0): float32(128 / 255) * 255 rounds to 128.0 exactly; a class
    outside the 21 colours stays black; the argmax form picks the lowest index on a tie."""
    lab = np.array([[[0, 1], [1, 0]], [[1, 1], [0, 25]]], np.int64)
    g = T.grid_model(lab, [0, 1], transform=L.TB_LABEL)
    red = np.zeros((6, 10), np.uint8)
    red[2, 3] = red[3, 2] = red[2, 6] = red[2, 7] = 128
    assert np.array_equal(g[:, :, 0], red) and not g[:, :, 1:].any()
    logits = np.zeros((2, 2, 2, 2), np.float32)
    logits[:, 1] = np.where(lab == 1, 1.0, -1.0)
    logits[1, :, 1, 1] = 0.5                                  # a tie -> class 0
    assert np.array_equal(T.grid_model(logits, [0, 1], c0=0, nc=2, transform=L.TB_ARGMAX), g)
    assert T.PALETTE.shape == (21, 3) and T.PALETTE[1].tolist() == [128, 0, 0] and T.PALETTE[20].tolist() == [0, 64, 128]


def test_tag_tables_and_sample_selection():
    assert T.tags('fundus') == ['train/Image', 'train/Image_Freq', 'train/Image_Rec', 'train/Soft_Predicted_OC', 'train/Soft_Predicted_OD',
                                'train/GT_OC', 'train/GT_OD']
    assert T.tags('prostate') == ['train/Image', 'train/Image_Freq', 'train/Image_Rec', 'train/Predicted', 'train/GT']
    assert [T.selected_samples('fundus', b) for b in (16, 9, 8, 5, 3)] == [[0, 4, 8], [0, 4, 8], [0, 4], [0, 4], [0]]
    assert [T.selected_samples('prostate', b) for b in (10, 7, 6, 4, 3)] == [[0, 3, 6], [0, 3, 6], [0, 3], [0, 3], [0]]
    assert [g[4] for g in T.TABLES['fundus']['grids']] == [True] * 5 + [False] * 2
    assert [g[4] for g in T.TABLES['prostate']['grids']] == [True] * 3 + [False] * 2
    assert T.grid_shape(3, 256, 256) == (260, 776) and T.grid_shape(1, 37, 53) == (37, 53)


def test_more_classes_than_colours_is_refused():
    import torch
    t = torch.zeros(1, 22, 2, 2)
    with pytest.raises(ValueError, match='21 colours'):
        T.describe(t, 'nchw', [0], 0, 22, L.TB_ARGMAX, False, 0)
    with pytest.raises(ValueError):
        T.describe(t, 'nchw', [1], 0, 3, L.TB_IDENTITY, True, 0)              # sample outside the batch


# ---------------------------------------------------------------------------------------------------------------- add_image
def _vint(n):
    """protobuf varint of a length below 2^14, spelled out."""
    assert 0 <= n < 1 << 14
    return bytes([n]) if n < 128 else bytes([n & 0x7f | 0x80, n >> 7])


def test_image_record_bytes_by_hand_and_round_trip(tmp_path):
    img = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]], [[1, 2, 3], [4, 5, 6], [7, 8, 9]]], np.uint8)      # 2 x 3
    h, w, cs, png = E.encode_png(img)
    assert (h, w, cs) == (2, 3, 3) and png[:8] == b'\x89PNG\r\n\x1a\n' and len(png) < 128
    ev = E.encode_event(12.5, step=7, images=[('t/x', h, w, cs, png)])
    image = b'\x08\x02' + b'\x10\x03' + b'\x18\x03' + b'\x22' + _vint(len(png)) + png                  # Image{1: 2, 2: 3, 3: 3, 4: png}
    value = b'\x0a\x03t/x' + b'\x22' + _vint(len(image)) + image                                      # Value{tag = 1, image = 4}
    summary = b'\x0a' + _vint(len(value)) + value                                                     # Summary{value = 1}
    want = b'\x09' + struct.pack('<d', 12.5) + b'\x10\x07' + b'\x2a' + _vint(len(summary)) + summary          # Event{1, 2, summary = 5}
    assert ev == want
    # through the writer and the reader, mixed with scalar records, in order
    wr = E.SummaryWriter(str(tmp_path))
    wr.add_scalar('lr', 0.5, 3)
    wr.add_image('t/x', img, 3)
    wr.add_scalar('lr', 0.25, 4)
    wr.add_image('t/gray', img[:, :, 0], 4)
    wr.close()
    evs = E.read_events(wr.path)
    assert [(e['step'], e['scalars'], [i[:4] for i in e['images']]) for e in evs[1:]] == [
        (3, [('lr', 0.5)], []), (3, [], [('t/x', 2, 3, 3)]), (4, [('lr', 0.25)], []), (4, [], [('t/gray', 2, 3, 1)])]
    assert np.array_equal(np.array(Image.open(io.BytesIO(evs[2]['images'][0][4]))), img)
    assert np.array_equal(np.array(Image.open(io.BytesIO(evs[4]['images'][0][4]))), img[:, :, 0])
    # a flipped byte inside the PNG is caught by the record's checksum
    data = bytearray(open(wr.path, 'rb').read())
    data[data.index(b'\x89PNG') + 20] ^= 0x40
    bad = tmp_path / 'bad'
    bad.write_bytes(bytes(data))
    with pytest.raises(ValueError, match='corrupt record'):
        E.read_events(str(bad))
    with pytest.raises(ValueError):
        E.encode_png(np.zeros((2, 2, 3), np.float32))


def test_queued_writer_keeps_the_order_of_the_calls(tmp_path):
    """The writer thread of --tb_images: scalars and images through one queue, images fetched lazily; close() drains."""
    img = np.arange(4 * 5 * 3, dtype=np.uint8).reshape(4, 5, 3)
    wr = E.QueuedWriter(str(tmp_path))
    fetched = []

    def fetch():
        fetched.append(1)
        return [('train/Image', img), ('train/GT', img[::-1])]
    wr.add_scalars_at(0, [('lr', 1.0), ('loss/a', 2.0)])
    wr.add_images_at(0, fetch)
    wr.add_scalars_at(2, [('lr', 0.5)])
    wr.close()
    evs = E.read_events(wr.path)
    assert fetched == [1] and wr.seconds['records'] == 2
    assert [(e['step'], [s[0] for s in e['scalars']], [i[0] for i in e['images']]) for e in evs[1:]] == [
        (0, ['lr'], []), (0, ['loss/a'], []), (0, [], ['train/Image']), (0, [], ['train/GT']), (2, ['lr'], [])]
    assert np.array_equal(np.array(Image.open(io.BytesIO(evs[4]['images'][0][4]))), img[::-1])
    # an error in the thread surfaces at close()
    wr = E.QueuedWriter(str(tmp_path / 'e'))
    wr.add_images_at(0, lambda: [('x', np.zeros((2, 2, 3), np.float32))])
    with pytest.raises(ValueError):
        wr.close()


# ---------------------------------------------------------------------------------------------------------------- rd_crc32c
def _native():
    import ctypes
    assert os.path.exists(L.LIB_PATH), 'build first: python -c "import __graft_entry__ as g; g.build()"'
    fn = ctypes.CDLL(L.LIB_PATH).rd_crc32c
    fn.restype, fn.argtypes = ctypes.c_uint32, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32]
    return lambda b, seed=0: fn(bytes(b), len(b), seed)


def test_native_crc32c_rfc3720_values_python_routine_and_chaining():
    crc = _native()
    # RFC 3720 B.4: 32 bytes of zeros, of ones, ascending, descending; and the classic check string
    assert crc(b'\x00' * 32) == 0x8A9136AA and crc(b'\xff' * 32) == 0x62A8AB43
    assert crc(bytes(range(32))) == 0x46DD794E and crc(bytes(range(31, -1, -1))) == 0x113FDB5C
    assert crc(b'123456789') == 0xE3069283 == E.crc32c(b'123456789')
    rng = np.random.RandomState(7)
    for n in (0, 1, 7, 8, 9, 4096, 100003):
        b = rng.randint(0, 256, n).astype(np.uint8).tobytes()
        want = E.crc32c(b)
        assert crc(b) == want, n
        for cut in sorted({0, n // 3, max(n - 1, 0), n}):
            assert crc(b[cut:], crc(b[:cut])) == want, (n, cut)                # seed chaining
        assert E.crc32c(b[n // 2:], E.crc32c(b[:n // 2])) == want
        assert E.crc32c_fast(b) == want                                        # what the writer calls (native from 64 bytes on)


# ---------------------------------------------------------------------------------------------------------------- the flag
def test_tb_images_flag_parses():
    import train
    base = ['--save_path', 'x']
    assert train.parse_args(base).tb_images == 0
    assert train.parse_args(base + ['--tb_images']).tb_images == 100
    assert train.parse_args(base + ['--tb_images', '2']).tb_images == 2
    assert train.parse_args(base + ['--tb_images', '--ram']).tb_images == 100


def test_struct_size_of_the_grid_descriptor(tmp_path):
    import ctypes
    import subprocess
    c = tmp_path / 's.c'
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ramdsir.h"\nint main(){printf("%zu %zu %zu %d %d %d\\n", sizeof(rd_tb_grid_t), '
                 'offsetof(rd_tb_grid_t, sample), offsetof(rd_tb_grid_t, slot), RD_TB_MAX_GRIDS, RD_TB_PALETTE, RD_TB_LABEL);return 0;}')
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    assert out == [ctypes.sizeof(L.RdTbGrid), L.RdTbGrid.sample.offset, L.RdTbGrid.slot.offset, L.TB_MAX_GRIDS, L.TB_PALETTE, L.TB_LABEL]
