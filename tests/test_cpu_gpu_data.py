"""CPU: the host side of train.py --gpu_data -- Pillow's resampling as integer tables (ramdsir/resample.py, the reference the
augmentation kernel is tested against), the parameter datasets' draws against the host path's datasets, the new descriptor
structs' layout, and the refusal of non-RGB images."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

import synth_data as SD
from ramdsir import resample as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pairs():
    rng = np.random.RandomState(7)
    pairs = [((800, 800), (256, 256))]
    pairs += [((256, 256), (m, 256)) for m in range(256, 385)] + [((256, 256), (256, m)) for m in range(256, 385)]
    pairs += [((300 - 4 * i, 280 + 8 * d), (256, 256)) for d in range(1, 5) for i in range(4)]       # synth_data vary=True sizes
    pairs += [(tuple(rng.randint(8, 1025, 2)), tuple(rng.randint(8, 1025, 2))) for _ in range(100)]
    return pairs


def test_bilinear_tables_match_pillow_bit_for_bit():
    rng = np.random.RandomState(0)
    for (w0, h0), (w1, h1) in _pairs():
        img = rng.randint(0, 256, (h0, w0, 3)).astype(np.uint8)
        ref = np.asarray(Image.fromarray(img).resize((w1, h1), Image.BILINEAR))
        assert np.array_equal(RS.resize_bilinear(img, w1, h1), ref), ((w0, h0), (w1, h1))


def test_nearest_tables_match_pillow_bit_for_bit():
    rng = np.random.RandomState(1)
    for (w0, h0), (w1, h1) in _pairs():
        m = rng.randint(0, 256, (h0, w0)).astype(np.uint8)
        ref = np.asarray(Image.fromarray(m).resize((w1, h1), Image.NEAREST))
        assert np.array_equal(RS.resize_nearest(m, w1, h1), ref), ((w0, h0), (w1, h1))


def test_identity_table_reproduces_its_input():
    """'No scaling' runs the S -> S tables in the kernel: they must be the identity (Pillow skips such a pass)."""
    xmin, cnt, k = RS.bilinear_coeffs(256, 256)
    x = np.random.RandomState(2).randint(0, 256, (256, 3)).astype(np.uint8)
    assert np.array_equal(RS.apply_pass(x[None], 256, 0)[0], x)
    assert (k.sum(1) == 1 << RS.PRECISION_BITS).all()


def _emulate_fundus(rec, size=256):
    """numpy integer pipeline of one FundusParams record == Fundus_Multi[i] under Resize + RandomScaleCrop."""
    from dataset.transform import fundus_mask
    ik, pk, sw, sh, cx, cy, lam = rec
    img = np.asarray(Image.open(ik))
    g = None
    for lst in [f for f in os.listdir(_emulate_fundus.base) if f.endswith('_train.list')]:
        for l in open(os.path.join(_emulate_fundus.base, lst)).read().split('\n'):
            if l and os.path.normpath(os.path.join(_emulate_fundus.base, l.split(' ')[0])) == ik:
                g = np.asarray(Image.open(os.path.join(_emulate_fundus.base, l.split(' ')[1])).convert('L'))
    a = RS.resize_bilinear(RS.resize_bilinear(img, size, size), sw, sh)[cy:cy + size, cx:cx + size]
    m = RS.resize_nearest(RS.resize_nearest(g, size, size), sw, sh)[cy:cy + size, cx:cx + size]
    p = RS.resize_bilinear(np.asarray(Image.open(pk)), size, size)
    return a, p, np.float32(lam), fundus_mask(m)


@pytest.mark.parametrize('out_domain', [True, False])
def test_fundus_params_reproduce_fundus_multi(tmp_path, out_domain):
    """Over whole lists: the parameter dataset draws what Fundus_Multi draws (same generators, same order) and the integer
    emulation of its record is that sample, bit for bit; both generators end in the same state."""
    import train as T
    from dataset.fundus import Fundus_Multi
    from ramdsir.gpu_data import FundusParams
    base = SD.make_fundus_tree(str(tmp_path), n_train=4, n_test=1, vary=True)
    _emulate_fundus.base = base
    tf = T.Compose([T.trans.Resize((256, 256)), T.trans.RandomScaleCrop((256, 256))])
    kw = dict(base_dir=base, split='train', domain_idx_list=[1, 2], is_out_domain=out_domain, test_domain_idx=0)
    host, par = Fundus_Multi(transform=tf, **kw), FundusParams(transform=tf, **kw)
    order = list(range(len(host))) * 3
    random.seed(11); np.random.seed(11)
    ref = [host[i] for i in order]
    st = (random.getstate(), np.random.get_state())
    random.seed(11); np.random.seed(11)
    recs = [par[i] for i in order]
    assert random.getstate() == st[0]
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), st[1]))
    assert any(r[2] != 256 for r in recs) and any(r[2] == 256 for r in recs)
    for (img, other, lam, mask), rec in zip(ref, recs):
        a, p, l, m = _emulate_fundus(rec)
        assert np.array_equal(img.numpy(), a) and np.array_equal(other.numpy(), p)
        assert float(lam) == l and np.array_equal(mask.numpy(), m)


@pytest.mark.parametrize('out_domain', [True, False])
def test_prostate_params_reproduce_prostate_multi(tmp_path, out_domain):
    from dataset.prostate import Prostate_Multi
    from ramdsir.gpu_data import ProstateParams
    base = SD.make_prostate_tree(str(tmp_path), n=4, S=32)
    kw = dict(base_dir=base, split='train', domain_idx_list=[1, 3], is_out_domain=out_domain, test_domain_idx=0)
    host, par = Prostate_Multi(**kw), ProstateParams(**kw)
    order = list(range(len(host))) * 3
    random.seed(5); np.random.seed(5)
    ref = [host[i] for i in order]
    st = (random.getstate(), np.random.get_state())
    random.seed(5); np.random.seed(5)
    recs = [par[i] for i in order]
    assert random.getstate() == st[0]
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), st[1]))
    for (img, other, lam, mask), (ik, pk, l) in zip(ref, recs):
        assert np.array_equal(img.numpy(), np.load(ik).astype(np.float32))
        assert np.array_equal(other.numpy(), np.load(pk).astype(np.float32))
        lab = torch.from_numpy(np.load(ik.replace(os.sep + 'image' + os.sep, os.sep + 'mask' + os.sep))).long()
        assert float(lam) == np.float32(l) and torch.equal(mask, lab)


def test_augment_struct_sizes_match_the_c_compiler(tmp_path):
    from ramdsir import _lib as L
    names = {'rd_aug_image_t': L.RdAugImage, 'rd_fundus_sample_t': L.RdFundusSample, 'rd_fundus_batch_t': L.RdFundusBatch,
             'rd_prostate_sample_t': L.RdProstateSample, 'rd_prostate_batch_t': L.RdProstateBatch}
    src = '#include <stdio.h>\n#include "ramdsir.h"\nint main(){' + ''.join(
        'printf("%s %%zu\\n", sizeof(%s));' % (n, n) for n in names) + 'printf("chunk %d\\n", RD_AUG_CHUNK); return 0;}'
    c = tmp_path / 's.c'
    c.write_text(src)
    exe = tmp_path / 's'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(c), '-o', str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    sizes = dict(zip(out[0::2], map(int, out[1::2])))
    for n, cls in names.items():
        assert ctypes.sizeof(cls) == sizes[n], n
    assert sizes['chunk'] == L.AUG_CHUNK


def test_non_rgb_image_is_refused_by_name(tmp_path):
    from ramdsir.gpu_data import FundusParams, FundusResident
    base = SD.make_fundus_tree(str(tmp_path), n_train=2, n_test=1, vary=True)
    bad = os.path.join(base, 'Domain3', 'train', 'ROIs', 'image', 'd3_train_01.png')
    Image.open(bad).convert('RGBA').save(bad)
    ds = FundusParams(base_dir=base, split='train', domain_idx_list=[1], is_out_domain=True, test_domain_idx=0)
    with pytest.raises(ValueError, match='d3_train_01.png has mode RGBA'):
        FundusResident([ds], workers=2)
