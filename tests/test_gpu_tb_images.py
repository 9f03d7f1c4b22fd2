"""-m gpu: train.py --tb_images -- rd_tb_grids (csrc/tb_grid.hip) against its numpy model (ramdsir/tb_images.py grid_model), the
fused step and the module trainer handing it the right buffers at the right time, and the CLI end to end.

Equality rules.  Identity, label and argmax grids: bit for bit (the same IEEE operations on both sides).  sigmoid / tanh grids: expf /
tanhf of the device and of numpy may differ in the last bits, which moves a value across a grey-level boundary now and then: every pixel
within ONE level of the model, at most 1 % of the pixels different at all (on the CPU the float32 pipeline against the float64 one, and
against a 4-ulp perturbation of it, differs on 0.015 - 0.06 % of such pixels, never by more than one level)."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import synth_data as SD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
H, W = 37, 53               # odd, H != W: stride and tile-offset errors show

from ramdsir import _lib as L, tb_images as T, step as S_       # noqa: E402


def _assert_exact(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()))


def _assert_close(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print('%s: %d of %d pixels differ, max %d' % (what, int((d > 0).sum()), d.size, int(d.max())))
    assert d.max() <= 1, (what, int(d.max()))
    assert (d > 0).mean() <= 0.01, (what, float((d > 0).mean()))


def _check(got, want, transform, what):
    (_assert_close if transform in (L.TB_SIGMOID, L.TB_TANH) else _assert_exact)(got, want, what)


def _run(specs):
    """specs as tb_images.compose takes them -> list of uint8 grids."""
    total = sum(3 * np.prod(T.grid_shape(len(s[2]), *_hw(s[0], s[1]))) for s in specs)
    out = torch.full((int(total) + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    ws = torch.empty(L.lib().rd_tb_grids_workspace(len(specs)) // 4, dtype=torch.float32, device=DEV)
    layout = T.compose(specs, out, ws)
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert (a[int(total):] == 0xAB).all()                   # nothing written behind the last grid
    return [a[off:off + gh * gw * 3].reshape(gh, gw, 3) for off, gh, gw in layout]


def _hw(t, layout):
    return {'nhwc': t.shape[1:3], 'nchw': t.shape[2:4], 'nhw': t.shape[1:3]}[layout]


def _nchw(t, layout):
    """The float32 NCHW (or integer NHW) numpy array the model takes."""
    if layout == 'nhw':
        return t.cpu().numpy()
    t = t.float()
    return (t.permute(0, 3, 1, 2) if layout == 'nhwc' else t).cpu().numpy()


def _make(layout_name, N, C, gen, scale=1.0):
    """A random source of N samples, C channels: 'nhwc8_f32' / 'nhwc8_bf16' (channel stride 8, the pad filled with junk that must not
    be read as data), 'nhwc4_f32' (one whole fp32 slot), 'nchw_f32'."""
    if layout_name.startswith('nhwc'):
        cs = int(layout_name[4])
        t = torch.randn(N, H, W, cs, generator=gen) * scale
        t[..., C:] = 1e4
        return t.to(torch.bfloat16 if layout_name.endswith('bf16') else torch.float32).to(DEV), 'nhwc'
    return (torch.randn(N, C, H, W, generator=gen) * scale).to(DEV), 'nchw'


CASES = [('fundus', 9), ('fundus', 5), ('fundus', 3), ('prostate', 7), ('prostate', 4)]


@pytest.mark.parametrize('layout_name', ['nhwc8_f32', 'nhwc8_bf16', 'nhwc4_f32', 'nchw_f32'])
@pytest.mark.parametrize('dataset,B', CASES)
def test_kernel_matches_the_model(layout_name, dataset, B):
    gen = torch.Generator().manual_seed(B * 7 + len(layout_name))
    samples = T.selected_samples(dataset, B)
    assert len(samples) == {9: 3, 5: 2, 3: 1, 7: 3, 4: 2}[B]
    img, lay = _make(layout_name, B, 3, gen)
    # argmax over 3 classes: a per-pixel permutation of three distinct values (exact in bf16), so that no two classes tie -- except
    # in ONE pixel, where classes 1 and 2 share the maximum and class 1 must win
    vals = torch.tensor([-1.0, 0.25, 1.5])
    perm = torch.argsort(torch.rand(B, H, W, 3, generator=gen), dim=-1)
    cls = vals[perm]
    cls[samples[0], 5, 7] = torch.tensor([-1.0, 3.0, 3.0])
    if lay == 'nhwc':
        logit = torch.full((B, H, W, img.shape[-1]), 1e4)
        logit[..., :3] = cls
        logit = logit.to(img.dtype).to(DEV)
    else:
        logit = cls.permute(0, 3, 1, 2).contiguous().to(DEV)
    specs = [(img, lay, samples, 0, 3, L.TB_IDENTITY, True), (img, lay, samples, 1, 1, L.TB_IDENTITY, True),
             (img, lay, samples, 2, 1, L.TB_IDENTITY, True), (logit, lay, samples, 0, 3, L.TB_ARGMAX, False)]
    for s in (0.5, 2.0):
        soft, _ = _make(layout_name, B, 3, gen, scale=s)
        specs += [(soft, lay, samples, 0, 1 if s == 0.5 else 3, L.TB_SIGMOID, True), (soft, lay, samples, 0 if s == 0.5 else 1, 3 if s == 0.5 else 1, L.TB_TANH, True)]
    grids = _run(specs)
    for i, (g, sp) in enumerate(zip(grids, specs)):
        t, l, smp, c0, nc, tr, norm = sp
        assert g.shape == T.grid_shape(len(samples), H, W) + (3,)
        _check(g, T.grid_model(_nchw(t, l), smp, c0, nc, tr, norm), tr, '%s grid %d' % (layout_name, i))
    am = grids[3]
    oy, ox = (5, 7) if len(samples) == 1 else (5 + 2, 7 + 2)
    assert am[oy, ox].tolist() == T.PALETTE[1].tolist()     # the tied pixel: the lowest index of the maximum


@pytest.mark.parametrize('dataset,B', CASES)
def test_label_and_plane_grids_are_exact(dataset, B):
    gen = torch.Generator().manual_seed(B)
    samples = T.selected_samples(dataset, B)
    lab = torch.randint(0, 4, (B, H, W), generator=gen)
    lab[samples[-1], 3, 4] = 21                             # outside the palette: black
    lab[samples[0], 0, 0] = 20
    lab = lab.to(DEV)
    planes = (torch.rand(B, 2, H, W, generator=gen) > 0.5).float().to(DEV)
    specs = [(lab, 'nhw', samples, 0, 1, L.TB_LABEL, False), (planes, 'nchw', samples, 0, 1, L.TB_IDENTITY, False),
             (planes, 'nchw', samples, 1, 1, L.TB_IDENTITY, False)]
    grids = _run(specs)
    for g, (t, l, smp, c0, nc, tr, norm) in zip(grids, specs):
        _assert_exact(g, T.grid_model(_nchw(t, l), smp, c0, nc, tr, norm), 'label / plane')
    assert set(np.unique(grids[1])) <= {0, 255} and set(np.unique(grids[2])) <= {0, 255}
    oy, ox = (0, 0) if len(samples) == 1 else (2, 2)
    assert grids[0][oy, ox].tolist() == [0, 64, 128]


def _step_like_sources(dataset, B, dtype, gen):
    """Tensors laid out as a TrainStep holds them: x [img ; img_freq] NHWC with the channel slot, logits (2B), rec logits (B), target."""
    cs = 8 if dtype == torch.bfloat16 else 4
    x = (torch.randn(2 * B, H, W, cs, generator=gen)).to(dtype).to(DEV)
    logits = (torch.randn(2 * B, H, W, cs, generator=gen) * 2).to(dtype).to(DEV)
    rec = (torch.randn(B, H, W, cs, generator=gen) * 0.5).to(dtype).to(DEV)
    if dataset == 'fundus':
        target = (torch.rand(B, 2, H, W, generator=gen) > 0.5).float().to(DEV)
    else:
        target = torch.randint(0, 2, (B, H, W), generator=gen).to(DEV)
    fundus = dataset == 'fundus'
    return {'img': (x[:B], 'nhwc', L.TB_IDENTITY), 'img_freq': (x[B:], 'nhwc', L.TB_IDENTITY), 'rec': (rec, 'nhwc', L.TB_TANH),
            'pred': (logits[:B], 'nhwc', L.TB_SIGMOID), 'pred_class': (logits[:B], 'nhwc', L.TB_ARGMAX),
            'target': (target, 'nchw' if fundus else 'nhw', L.TB_IDENTITY), 'label': (target, 'nhw', L.TB_LABEL)}


def _model_grids(comp, sources):
    return [T.grid_model(_nchw(t, lay), smp, c0, nc, tr, norm) for t, lay, smp, c0, nc, tr, norm in comp.specs(sources)]


def _compare(comp, images, sources, what):
    assert [t for t, _ in images] == T.tags(comp.dataset)
    for (tag, g), want, sp in zip(images, _model_grids(comp, sources), comp.specs(sources)):
        _check(g, want, sp[5], '%s %s' % (what, tag))


@pytest.mark.parametrize('dataset,B,dtype', [('fundus', 9, torch.bfloat16), ('prostate', 7, torch.bfloat16), ('fundus', 5, torch.float32)])
def test_all_grids_of_a_dataset_in_one_call(dataset, B, dtype):
    """The seven Fundus / five Prostate grids as ONE descriptor array, through the composer train.py uses (pinned staging, event)."""
    gen = torch.Generator().manual_seed(11)
    sources = _step_like_sources(dataset, B, dtype, gen)
    comp = T.GridComposer(dataset, B, H, W, 2, DEV)
    pending = comp.enqueue(sources)
    images = pending.images()
    assert len(images) == {'fundus': 7, 'prostate': 5}[dataset]
    _compare(comp, images, sources, dataset)


def test_invalid_records_are_refused_before_any_launch():
    t = torch.zeros(2, 3, 4, 4, device=DEV)
    out = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(1024, dtype=torch.float32, device=DEV)
    g = T.describe(t, 'nchw', [0, 1], 0, 3, L.TB_IDENTITY, True, out.data_ptr())
    lib = L.lib()
    st = torch.cuda.current_stream().cuda_stream
    for field, v in (('n', 4), ('n', 0), ('nc', 2), ('transform', 9), ('etype', 2), ('H', 0)):
        bad = L.RdTbGrid.from_buffer_copy(g)
        setattr(bad, field, v)
        assert lib.rd_tb_grids(bad, 1, ws.data_ptr(), 4096, st) == -1, field
    assert lib.rd_tb_grids(g, 1, ws.data_ptr(), 8, st) == -1                    # workspace too small
    assert lib.rd_tb_grids(g, 9, ws.data_ptr(), 4096, st) == -1
    torch.cuda.synchronize()
    assert not out.any()


# ------------------------------------------------------------------------------------------------------------- the fused step
def _trainstep(dataset, dtype, bs, S):
    bank, mods = S_.make_bank(DEV, 3, 16, 2, len(bs))
    g = torch.Generator().manual_seed(1)
    for (m, k), (off, shape) in bank.index.items():
        v = bank.p(m, k)
        if len(shape) == 4:
            v.copy_((torch.randn(shape, generator=g) * (2.0 / (shape[0] * shape[2] * shape[3])) ** 0.5).to(DEV))
        elif '.bn' in k and k.endswith('weight'):
            v.fill_(1.0)
    ts = S_.TrainStep(bank, mods, dtype, bs, S, S, dataset=dataset, consistency='kd', lr=1e-3, total_iters=100,
                      ram='u8' if dataset == 'fundus' else True)
    ts.wpack.refresh()
    return bank, ts


def _batches(dataset, B, S, n=2):
    gen = torch.Generator(device=DEV).manual_seed(5)
    out = []
    for i in range(n):
        if dataset == 'fundus':
            src = (torch.rand(B, S, S, 3, device=DEV, generator=gen) * 255).to(torch.uint8)
            trg = (torch.rand(B, S, S, 3, device=DEV, generator=gen) * 255).to(torch.uint8)
            tgt = (torch.rand(B, 2, S, S, device=DEV, generator=gen) > 0.5).float()
        else:
            src = torch.rand(B, S, S, 3, device=DEV, generator=gen) * 2 - 1
            trg = torch.rand(B, S, S, 3, device=DEV, generator=gen) * 2 - 1
            tgt = (torch.rand(B, S, S, device=DEV, generator=gen) > 0.7).long()
        lam = torch.tensor([0.1 * (1 + (i + j) % 9) for j in range(B)], device=DEV)
        out.append((src, trg, lam, tgt))
    return out


def _arm(ts, comp, box):
    ts.arm_after_step(lambda slot: box.append(comp.enqueue(T.train_step_sources(ts, slot))))


@pytest.mark.parametrize('dataset,dtype', [('fundus', torch.bfloat16), ('prostate', torch.bfloat16), ('fundus', torch.float32)])
def test_fused_step_composes_the_batch_it_trained_on(dataset, dtype):
    """Trainer A: a PIPELINED step (the next batch is mixed into the other input slot while it runs) with the grids armed, then the
    upload of the next mask, as train.py orders them.  Twin B (same parameters): the classical step on the same batch; its x, logits,
    rec_logits and target, read afterwards, go through the model.  A's grids must be B's -- and must NOT be those of the next batch
    (the other input slot, the next mask).  Then: two armed steps leave the parameters of two unarmed steps, bit for bit."""
    bs, S = [3, 3, 3], 32
    B = sum(bs)
    batches = _batches(dataset, B, S)
    bank_a, A = _trainstep(dataset, dtype, bs, S)
    bank_b, Bt = _trainstep(dataset, dtype, bs, S)
    assert torch.equal(bank_a.params, bank_b.params)
    comp = T.GridComposer(dataset, B, S, S, 2, DEV)
    box = []
    A.load_raw(*batches[0][:3])
    A.load_target(batches[0][3])
    _arm(A, comp, box)
    A.load_raw_next(*batches[1][:3])
    A.step()
    A.load_target(batches[1][3])
    assert len(box) == 1 and A._after_step is None
    images = box[0].images()
    Bt.load_raw(*batches[0][:3])
    Bt.load_target(batches[0][3])
    Bt.step()
    torch.cuda.synchronize()
    src_b = {k: (v[0].clone(), v[1], v[2]) for k, v in T.train_step_sources(Bt, Bt._slot).items()}
    _compare(comp, images, src_b, 'step 0')
    # the second step: A on the batch it mixed during the first (armed again), B classically
    _arm(A, comp, box)
    A.step()
    Bt.load_raw(*batches[1][:3])
    Bt.load_target(batches[1][3])
    Bt.step()
    torch.cuda.synchronize()
    src_b1 = T.train_step_sources(Bt, Bt._slot)
    images1 = box[1].images()
    _compare(comp, images1, src_b1, 'step 1')
    by_tag0, by_tag1 = dict(images), dict(images1)
    gt = [t for t in T.tags(dataset) if 'GT' in t]
    for tag in ['train/Image', 'train/Image_Freq'] + gt:
        assert not np.array_equal(by_tag0[tag], by_tag1[tag]), tag              # not the other slot, not the next mask
    for g in gt:
        assert set(np.unique(by_tag0[g])) <= ({0, 255} if dataset == 'fundus' else {0, 128})
    assert torch.equal(bank_a.params, bank_b.params) and torch.equal(bank_a.exp_avg_sq, bank_b.exp_avg_sq)
    assert torch.equal(A.losses, Bt.losses) and int(A.iter) == 2


def test_arming_a_captured_graph_is_refused():
    bank, ts = _trainstep('fundus', torch.bfloat16, [1, 1, 1], 32)
    ts.graph = object()                                     # (what capture() leaves; nothing is replayed here)
    with pytest.raises(RuntimeError, match='hipGraph'):
        ts.arm_after_step(lambda slot: None)


# ------------------------------------------------------------------------------------------------------------- the module trainer
def test_module_trainer_composes_its_own_tensors():
    sys.path.insert(0, os.path.join(ROOT, 'ram-dsir_amd'))
    from networks.unet import Encoder, Decoder, Rec_Decoder
    from ramdsir import trainer as TR
    torch.manual_seed(3)
    bs, S = [3, 3, 3], 32
    B = sum(bs)
    enc, dec = Encoder(c=3, norm='gn').cuda(), Decoder(num_classes=2, norm='gn').cuda()
    rec = Rec_Decoder(num_classes=3, norm='dsbn', num_domains=3).cuda()
    for m in (enc, dec, rec):
        m.train()
    tr = TR.ModuleTrainer(enc, dec, rec, bs, S, S, dataset='fundus', consistency='kd', lr=1e-3, total_iters=10, dtype=torch.float32)
    src, trg, lam, tgt = _batches('fundus', B, S, n=1)[0]
    seen = {}
    orig = T.module_sources

    def spy(*a):
        seen['src'] = orig(*a)
        return seen['src']
    T.module_sources = spy
    try:
        tr.arm_tb_images()
        tr.step(src, trg, lam, tgt)
    finally:
        T.module_sources = orig
    pending = tr.take_tb_images()
    with pytest.raises(RuntimeError):
        tr.take_tb_images()
    images = pending.images()
    img = seen['src']['img'][0]
    assert img.shape == (B, 3, S, S) and img.dtype == torch.float32 and seen['src']['rec'][0].shape == (B, 3, S, S)
    _compare(tr._tb, images, seen['src'], 'module trainer')
    assert all(g.shape == (S + 4, 3 * (S + 2) + 2, 3) for _, g in images)
    tr.step(src, trg, lam, tgt)                             # not armed: nothing pending
    assert tr._tb_pending is None


# ------------------------------------------------------------------------------------------------------------- the CLI
def _train(data, out, dataset, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, 'ram-dsir_amd', 'train.py'), '--data_root', data, '--dataset', dataset, '--domain_idxs',
           '1,2,3' if dataset == 'fundus' else '1,2,3,4,5', '--test_domain_idx', '0', '--ram', '--rec', '--is_out_domain', '--consistency',
           '--consistency_type', 'kd', '--save_path', out, '--epochs', '5', '--max_iters', '5', '--num_workers', '0', '--deterministic']
    return subprocess.run(cmd + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)


@pytest.mark.parametrize('dataset', ['fundus', 'prostate'])
def test_train_cli_tb_images(tmp_path, dataset):
    """train.py --tb_images 2 for five iterations: the scalar records of the default run plus, at iterations 0, 2 and 4, the image
    tags in the reference's order; every PNG is a 3-channel grid of the expected size; the ground truth is two-valued; the trained
    model does not depend on the flag; without the flag the file holds exactly the scalar records."""
    sys.path.insert(0, os.path.join(ROOT, 'ram-dsir_amd'))
    from utils import tfevents
    data = str(tmp_path / 'data')
    if dataset == 'fundus':
        SD.make_fundus_tree(data, n_train=8, n_test=1, hw=(72, 80), vary=False)
        scalar_tags = ['lr', 'loss/loss_bce_1', 'loss/loss_dice_1', 'loss/loss_bce_2', 'loss/loss_dice_2', 'loss/loss_consistency', 'loss/loss_rec']
        shape = T.grid_shape(3, 256, 256)                   # batch 3 + 6 + 7: samples 0, 4, 8 at the training size
    else:
        SD.make_prostate_tree(data, n=4, S=64)
        scalar_tags = ['lr', 'loss/loss_ce_1', 'loss/loss_dice_1', 'loss/loss_ce_2', 'loss/loss_dice_2', 'loss/loss_consistency', 'loss/loss_rec']
        shape = T.grid_shape(3, 64, 64)                     # batch 5 x 2: samples 0, 3, 6
    runs = {}
    for name, extra in (('plain', []), ('images', ['--tb_images', '2'])):
        out = str(tmp_path / name)
        r = _train(data, out, dataset, extra)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
        logs = os.listdir(os.path.join(out, 'log'))
        assert len(logs) == 1
        runs[name] = (torch.load(os.path.join(out, 'final_model.pth'), map_location='cpu'), tfevents.read_events(os.path.join(out, 'log', logs[0])))
    ck0, ev0 = runs['plain']
    ck1, ev1 = runs['images']
    for part in ck0:
        assert list(ck0[part]) == list(ck1[part])
        for k in ck0[part]:
            assert torch.equal(ck0[part][k], ck1[part][k]), (part, k)
    # the default run: the scalars of iteration 0 (--log_every 20), nothing else
    assert [(e['step'], e['scalars'][0][0]) for e in ev0[1:]] == [(0, t) for t in scalar_tags]
    assert all(not e['images'] for e in ev0)
    want = [(0, t) for t in scalar_tags] + [(it, t) for it in (0, 2, 4) for t in T.tags(dataset)]
    assert [(e['step'], (e['scalars'] or e['images'])[0][0]) for e in ev1[1:]] == want
    assert [e['scalars'] for e in ev1[1:8]] == [e['scalars'] for e in ev0[1:8]]          # the same values, too
    for e in ev1[8:]:
        tag, h, w, cs, png = e['images'][0]
        a = np.array(Image.open(io.BytesIO(png)))
        assert (h, w, cs) == shape + (3,) and a.shape == shape + (3,), (tag, h, w, cs, a.shape)
        if 'GT' in tag:
            assert set(np.unique(a)) <= ({0, 255} if dataset == 'fundus' else {0, 128}), tag
            assert a.any()
        elif tag != 'train/Predicted':
            assert a.min() == 0 and a.max() == 255, tag      # normalised over the selection
