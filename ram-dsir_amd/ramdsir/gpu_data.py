"""GPU-resident training data (train.py --gpu_data).

Every image and mask training can touch is decoded ONCE and kept in device memory; per step the host only draws the random
numbers -- the parameter datasets below make exactly the draws of dataset.fundus.Fundus_Multi (with train.py's
Resize(256) + RandomScaleCrop(256)) and dataset.prostate.Prostate_Multi, from the same generators in the same order -- and ONE
launch (rd_fundus_batch / rd_prostate_batch, csrc/augment.hip) makes the step's whole batch from them.  Pillow's 8-bit
resampling is integer arithmetic (ramdsir/resample.py), so the batches are bit-identical to the host path's with
--num_workers 0 (a run with worker processes draws in per-worker-seeded processes instead).

The parameter datasets go through train.py's own DataLoader / sampler / itertools.cycle construction with num_workers=0 and
`collate` (the records of a batch as a list); FundusResident.on_device / ProstateResident.on_device replace train.py's
on_device() for the per-domain batches of one step.
"""
import ctypes as C
import os
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Dataset

from ramdsir import _lib as L, resample as RS
from ramdsir._lib import _stream

FUNDUS_DOMAINS = ['Domain1', 'Domain2', 'Domain3', 'Domain4']            # dataset/fundus.py DOMAINS
PROSTATE_DOMAINS = ['Domain1', 'Domain2', 'Domain3', 'Domain4', 'Domain5', 'Domain6']
MEM_SHARE = 0.5             # the resident data may take at most this share of the device memory free at preload
LDS_TARGET = 80 * 1024      # rd_fundus_batch: the largest band of rows whose LDS fits here (two workgroups per CU)


def _read_list(path):
    with open(path, 'r') as f:
        return [l.replace('\n', '') for l in f.readlines()]


def collate(batch):
    """DataLoader collate_fn of the parameter datasets: the records as they are."""
    return list(batch)


class FundusParams(Dataset):
    """Fundus_Multi (split 'train', is_freq) under Resize((S, S)) + RandomScaleCrop((S, S)), draws only.  Record:
    (image path, partner path, sw, sh, cx, cy, lam)."""

    def __init__(self, domain_idx_list=None, base_dir=None, split='train', num=None, transform=None, is_freq=True,
                 is_out_domain=False, test_domain_idx=None, size=256):
        assert split == 'train' and is_freq, 'the parameter dataset covers the training split'
        self.base_dir, self.size = base_dir, size
        self.domain_name = list(FUNDUS_DOMAINS)
        self.domain_idx_list, self.is_out_domain, self.test_domain_idx = domain_idx_list, is_out_domain, test_domain_idx
        self.id_path = []
        for d in domain_idx_list:
            self.id_path += _read_list(os.path.join(base_dir, '%s_train.list' % self.domain_name[d]))
        if num is not None:
            self.id_path = self.id_path[:num]
        self._partner_lists = {}
        print('total {} samples'.format(len(self.id_path)))

    def __len__(self):
        return len(self.id_path)

    def partner_domains(self):
        return [d for d in self.domain_name if d != self.domain_name[self.test_domain_idx]]

    def __getitem__(self, index):
        id = self.id_path[index]
        S = self.size
        sw = sh = S
        if random.random() > 0.5:                                         # transform.py:186-194 on the S x S image
            sw = int(random.uniform(1, 1.5) * S)
            sh = int(random.uniform(1, 1.5) * S)
        cx = random.randint(0, sw - S)                                    # RandomCrop: x, then y
        cy = random.randint(0, sh - S)
        cur_domain_name = id.split(' ')[0].split('/')[0]
        domain_list = self.partner_domains()
        if self.is_out_domain:
            domain_list.remove(cur_domain_name)
        other = np.random.choice(domain_list, 1)[0]                       # fundus.py:205
        if other not in self._partner_lists:
            self._partner_lists[other] = _read_list(os.path.join(self.base_dir, other, 'train.list'))
        other_id = np.random.choice(self._partner_lists[other]).split(' ')[0]          # fundus.py:208
        lam = random.randint(1, 10) / 10                                  # fundus.py:35
        return (_key(self.base_dir, id.split(' ')[0]), _key(self.base_dir, other, other_id), sw, sh, cx, cy, lam)


class ProstateParams(Dataset):
    """Prostate_Multi (split 'train', is_freq), draws only.  Record: (slice path, partner path, lam)."""

    def __init__(self, domain_idx_list=None, base_dir=None, split='train', num=None, transform=None, is_freq=True,
                 is_out_domain=False, test_domain_idx=None):
        assert split == 'train' and is_freq, 'the parameter dataset covers the training split'
        self.base_dir, self.domain_name = base_dir, list(PROSTATE_DOMAINS)
        self.domain_idx_list, self.is_out_domain, self.test_domain_idx = domain_idx_list, is_out_domain, test_domain_idx
        self.id_path = []
        for d in domain_idx_list:
            lst = os.listdir(os.path.join(base_dir, self.domain_name[d], 'image'))
            self.id_path += [self.domain_name[d] + '/image/' + i for i in lst]
        if num is not None:
            self.id_path = self.id_path[:num]
        self._listing = {}
        print('total {} samples'.format(len(self.id_path)))

    def __len__(self):
        return len(self.id_path)

    def partner_domains(self):
        return [d for d in self.domain_name if d != self.domain_name[self.test_domain_idx]]

    def listing(self, domain):
        """os.listdir of a domain's slices, read once (the host path lists the directory at every draw: same order)."""
        if domain not in self._listing:
            self._listing[domain] = os.listdir(os.path.join(self.base_dir, domain, 'image'))
        return self._listing[domain]

    def __getitem__(self, index):
        id = self.id_path[index]
        domain_list = self.partner_domains()
        if self.is_out_domain:
            domain_list.remove(id.split('/')[0])
        other_domain_name = np.random.choice(domain_list, 1)[0]          # prostate.py:182
        other_id = np.random.choice(self.listing(other_domain_name))
        lam = random.randint(1, 10) / 10
        return (_key(self.base_dir, id), _key(self.base_dir, other_domain_name, 'image', other_id), lam)


def _key(*parts):
    return os.path.normpath(os.path.join(*parts))


def _pool(workers):
    return ThreadPoolExecutor(max_workers=min(16, max(1, int(workers))))


def _check_memory(nbytes, device, what):
    free = torch.cuda.mem_get_info(device)[0]
    if nbytes > MEM_SHARE * free:
        raise RuntimeError('--gpu_data: the resident %s data takes %.2f GB, more than %d %% of the %.2f GB free on %s; train without '
                           '--gpu_data' % (what, nbytes / 1e9, int(MEM_SHARE * 100), free / 1e9, device))


def _rgb_size(path):
    with Image.open(path) as im:
        if im.mode != 'RGB':
            raise ValueError('--gpu_data: %s has mode %s; the resident path holds RGB images only (train without --gpu_data)'
                             % (path, im.mode))
        return im.size


class FundusResident:
    """Decoded Fundus images (+ gray masks of the training lists' images) in device memory, the resampling tables, and the
    one-launch batch maker."""

    def __init__(self, datasets, workers=8, device=None, size=256):
        self.S = size
        base = datasets[0].base_dir
        masks = {}
        for ds in datasets:
            for line in ds.id_path:
                ip, mp = line.split(' ')[0], line.split(' ')[1]
                masks[_key(base, ip)] = _key(base, mp)
        partners = []
        for d in datasets[0].partner_domains():
            partners += [_key(base, d, l.split(' ')[0]) for l in _read_list(os.path.join(base, d, 'train.list'))]
        keys = list(dict.fromkeys(list(masks) + partners))
        with _pool(workers) as ex:
            sizes = list(ex.map(_rgb_size, keys))                          # headers only: modes checked before anything is decoded
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.device = device
        self.slot = {k: i for i, k in enumerate(keys)}
        offs, moffs, po, mo = [], [], 0, 0
        for k, (w, h) in zip(keys, sizes):
            offs.append(po)
            po += w * h * 3
            moffs.append(mo if k in masks else -1)
            mo += w * h if k in masks else 0
        _check_memory(po + mo, device, 'Fundus')
        self.pixels = torch.empty(max(po, 1), dtype=torch.uint8, device=device)
        self.masks = torch.empty(max(mo, 1), dtype=torch.uint8, device=device)

        def decode(i):
            k = keys[i]
            with Image.open(k) as im:
                img = np.array(im)
            m = None
            if k in masks:
                with Image.open(masks[k]) as mm:
                    m = np.array(mm.convert('L'))
                if m.shape != img.shape[:2]:
                    raise ValueError('--gpu_data: mask %s is %s, its image %s %s' % (masks[k], m.shape, k, img.shape[:2]))
            return i, img, m
        with _pool(workers) as ex:
            for i, img, m in ex.map(decode, range(len(keys))):
                self.pixels[offs[i]:offs[i] + img.size].copy_(torch.from_numpy(np.ascontiguousarray(img).reshape(-1)))
                if m is not None:
                    self.masks[moffs[i]:moffs[i] + m.size].copy_(torch.from_numpy(np.ascontiguousarray(m).reshape(-1)))

        T = RS.TableSet()
        S = size
        imgs = (L.RdAugImage * len(keys))()
        for i, (w, h) in enumerate(sizes):
            imgs[i].off, imgs[i].mask_off, imgs[i].h, imgs[i].w = offs[i], moffs[i], h, w
            imgs[i].tab_x, imgs[i].tab_y = T.offset(w, S, 0), T.offset(h, S, 1)
        self.stage2 = {m: (T.offset(S, m, 0), T.offset(S, m, 1)) for m in range(S, int(1.5 * S) + 1)}
        # LDS bounds of a band (csrc/augment.hip): stage-1 rows any band of R output rows reads, source rows those read
        heights = sorted(set(h for _, h in sizes))
        for R in (16, 8, 4, 2, 1):
            mid = max(RS.max_window(S, m, R) for m in self.stage2)
            src = max(RS.max_window(h, S, mid) for h in heights)
            lds = (src + 2 * mid) * S * 3
            if lds <= LDS_TARGET:
                break
        if lds > 160 * 1024:
            raise ValueError('--gpu_data: images of height %d need %d KiB of LDS per row band' % (heights[-1], lds // 1024))
        self.images = torch.from_numpy(np.frombuffer(bytes(imgs), np.uint8).copy()).to(device)
        self.tables = torch.from_numpy(T.array()).to(device)
        self.desc = L.RdFundusBatch(pixels=self.pixels.data_ptr(), masks=self.masks.data_ptr(), images=self.images.data_ptr(),
                                    tables=self.tables.data_ptr(), n_images=len(keys), S=S, id_x=self.stage2[S][0],
                                    id_y=self.stage2[S][1], band_rows=R, src_rows=src, mid_rows=mid)
        self.hw = (S, S)
        self.nbytes = po + mo

    def on_device(self, batches):
        """(src, trg, lam, mask) of one step from the per-domain record lists, concatenated in domain order: one launch."""
        recs = [r for b in batches for r in b]
        n, S = len(recs), self.S
        arr = (L.RdFundusSample * n)()
        for e, (ik, pk, sw, sh, cx, cy, lam) in zip(arr, recs):
            e.img, e.partner = self.slot[ik], self.slot[pk]
            e.tab_x, e.tab_y = self.stage2[sw][0], self.stage2[sh][1]
            e.sw, e.sh, e.cx, e.cy, e.lam = sw, sh, cx, cy, lam
        dev = self.device
        src = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
        trg = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
        lam = torch.empty((n,), dtype=torch.float32, device=dev)
        mask = torch.empty((n, 2, S, S), dtype=torch.float32, device=dev)
        d = L.RdFundusBatch.from_buffer_copy(self.desc)
        d.src, d.trg, d.lam, d.mask = src.data_ptr(), trg.data_ptr(), lam.data_ptr(), mask.data_ptr()
        L.check(L.lib().rd_fundus_batch(C.byref(d), arr, n, _stream()), 'rd_fundus_batch')
        return src, trg, lam, mask


def _slice_shape(path):
    return np.load(path, mmap_mode='r').shape


class ProstateResident:
    """The fp32 (S, S, 3) slices of every training and partner domain (+ the labels of the training lists' slices) in device
    memory, and the one-launch gather."""

    def __init__(self, datasets, workers=8, device=None):
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.device = device
        base = datasets[0].base_dir
        with_mask = {_key(base, i): _key(base, i.replace('image', 'mask')) for ds in datasets for i in ds.id_path}     # prostate.py:177
        keys = list(dict.fromkeys([_key(base, i) for ds in datasets for i in ds.id_path] +
                                  [_key(base, d, 'image', f) for d in datasets[0].partner_domains() for f in datasets[0].listing(d)]))
        with _pool(workers) as ex:
            shapes = list(ex.map(_slice_shape, keys))
        if len(set(shapes)) != 1 or len(shapes[0]) != 3 or shapes[0][2] != 3 or shapes[0][0] != shapes[0][1]:
            raise ValueError('--gpu_data: the Prostate slices must all be (S, S, 3); found %s' % sorted(set(shapes)))
        S = shapes[0][0]
        _check_memory(len(keys) * S * S * 13, device, 'Prostate')
        self.slot = {k: i for i, k in enumerate(keys)}
        self.slices = torch.empty((len(keys), S, S, 3), dtype=torch.float32, device=device)
        self.masks = torch.zeros((len(keys), S, S), dtype=torch.uint8, device=device)

        def decode(i):
            k = keys[i]
            img = np.load(k).astype(np.float32)
            m = None
            if k in with_mask:
                m = torch.from_numpy(np.load(with_mask[k])).long()
                if m.shape != (S, S) or int(m.min()) < 0 or int(m.max()) > 255:
                    raise ValueError('--gpu_data: labels of %s must be (S, S) in 0..255' % k)
            return i, img, m
        with _pool(workers) as ex:
            for i, img, m in ex.map(decode, range(len(keys))):
                self.slices[i].copy_(torch.from_numpy(img))
                if m is not None:
                    self.masks[i].copy_(m.to(torch.uint8))
        self.S, self.hw = S, (S, S)
        self.desc = L.RdProstateBatch(slices=self.slices.data_ptr(), masks=self.masks.data_ptr(), n_slices=len(keys), S=S)
        self.nbytes = len(keys) * S * S * 13

    def on_device(self, batches):
        recs = [r for b in batches for r in b]
        n, S = len(recs), self.S
        arr = (L.RdProstateSample * n)()
        for e, (ik, pk, lam) in zip(arr, recs):
            e.img, e.partner, e.lam = self.slot[ik], self.slot[pk], lam
        dev = self.device
        src = torch.empty((n, S, S, 3), dtype=torch.float32, device=dev)
        trg = torch.empty((n, S, S, 3), dtype=torch.float32, device=dev)
        lam = torch.empty((n,), dtype=torch.float32, device=dev)
        mask = torch.empty((n, S, S), dtype=torch.int64, device=dev)
        d = L.RdProstateBatch.from_buffer_copy(self.desc)
        d.src, d.trg, d.lam, d.mask = src.data_ptr(), trg.data_ptr(), lam.data_ptr(), mask.data_ptr()
        L.check(L.lib().rd_prostate_batch(C.byref(d), arr, n, _stream()), 'rd_prostate_batch')
        return src, trg, lam, mask


PARAMS = {'fundus': FundusParams, 'prostate': ProstateParams}


def preload(dataset, datasets, workers=8, device=None):
    """The resident store for train.py's parameter datasets (one per training domain)."""
    return (FundusResident if dataset == 'fundus' else ProstateResident)(datasets, workers=workers, device=device)
