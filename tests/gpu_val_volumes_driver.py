"""Driver of tests/test_gpu_gpu_val_volumes.py (TEST INFRASTRUCTURE, run as a script in a process of its own): train.py's
test_prostate and test_prostate_gpu on the same modules with a fixed checkpoint; prints one JSON line.

    python tests/gpu_val_volumes_driver.py <data_root>/prostate <domain index> <checkpoint> <output dir> <batch size>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ram-dsir_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch


def main(data_dir, dom, ck_path, out_dir, bs):
    import train
    from networks.unet import Encoder, Decoder
    from ramdsir import gpu_val_volumes as V
    from utils import prostate_eval as PE
    os.makedirs(os.path.join(out_dir, 'host'), exist_ok=True)
    os.makedirs(os.path.join(out_dir, 'gpu'), exist_ok=True)
    ck = torch.load(ck_path, map_location='cpu')
    enc, dec = Encoder().cuda(), Decoder(num_classes=2).cuda()
    enc.load_state_dict(ck['encoder_state_dict'])
    dec.load_state_dict(ck['seg_decoder_state_dict'])
    before = {k: v.clone() for m in (enc, dec) for k, v in m.state_dict().items()}
    rng_before = (torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone(), np.random.get_state()[1].copy())
    res = V.preload(data_dir, PE.DOMAIN_LIST[dom], batch_size=bs)
    assert res is not None, '--gpu_val_volumes: the volumes do not fit in device memory'
    ret_gpu = train.test_prostate_gpu(enc, dec, 3, res, dom, os.path.join(out_dir, 'gpu'), bs)
    untouched = all(torch.equal(v, before[k]) for m in (enc, dec) for k, v in m.state_dict().items())
    untouched = untouched and torch.equal(torch.get_rng_state(), rng_before[0]) and torch.equal(torch.cuda.get_rng_state(), rng_before[1])
    untouched = untouched and np.array_equal(np.random.get_state()[1], rng_before[2])
    ret_host = train.test_prostate(enc, dec, 3, data_dir, dom, os.path.join(out_dir, 'host'), bs)
    # per volume: the GPU path's volumes and Dice, and the host path's computed step by step as evaluate_domain does
    keep = {}
    dice_gpu = V.validate(enc, dec, res, bs, keep=keep)
    enc.eval()
    dec.eval()
    dice_host, same_post, same_pred, ties, shapes, dtypes, empty_gt, foreground = [], [], [], [], [], [], [], []
    with torch.no_grad():
        for i, file_name in enumerate(res.files):
            logits = []

            def forward(v):
                lg = dec(enc(v.cuda()))
                logits.append(lg)
                return lg
            image, mask = PE.load_case(data_dir, PE.DOMAIN_LIST[dom], file_name)
            post, mask = PE.predict_volume(forward, image, mask, bs)
            dice_host.append(PE.dc(post.astype(bool), mask.astype(bool)))
            # tie voxels: different logits whose fp32 softmax probabilities are equal (torch's argmax then says class 0)
            n_tie = 0
            gt_empty = np.array([np.sum(mask[jj]) == 0 for jj in range(mask.shape[0])], dtype=np.uint8)
            model_pred = np.zeros(mask.shape, np.uint8)
            for frames, lg in zip(V.frame_batches(mask.shape[0], bs), logits):
                sm = torch.softmax(lg, dim=1)
                n_tie += int(((sm[:, 0] == sm[:, 1]) & (lg[:, 0] != lg[:, 1])).sum())
                V.argmax_model(lg.cpu().numpy(), frames, gt_empty, model_pred)
            ties.append(n_tie)
            same_pred.append(bool(np.array_equal(model_pred, keep['pred'][i])))
            same_post.append(bool(np.array_equal(post.astype(np.uint8), keep['post'][i])))
            shapes.append(list(mask.shape))
            dtypes.append(str(np.asarray(image).dtype))
            empty_gt.append(int(gt_empty.sum()))
            foreground.append(float(keep['pred'][i].mean()))
    csv = [open(os.path.join(out_dir, d, '%d_val_log.csv' % dom)).read() for d in ('host', 'gpu')]
    print('RESULT ' + json.dumps(dict(ret_host=ret_host, ret_gpu=ret_gpu, dice_host=dice_host, dice_gpu=dice_gpu, same_post=same_post,
                                      same_pred=same_pred, ties=ties, shapes=shapes, dtypes=dtypes, empty_gt=empty_gt,
                                      foreground=foreground, untouched=untouched, csv=csv, files=list(res.files))))


if __name__ == '__main__':
    main(sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5]))
