"""Driver of tests/test_gpu_gpu_val.py (TEST INFRASTRUCTURE, run as a script in a process of its own): train.py's test_fundus and
test_fundus_gpu on the same modules with a fixed checkpoint; prints one JSON line.  Like train.main it starts the host path's loader
workers and pool BEFORE the first GPU call of the process.

    python tests/gpu_val_driver.py <data_root>/fundus <checkpoint> <output dir> <batch size>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'ram-dsir_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch
import torch.nn.functional as F


def main(data_dir, ck_path, out_dir, bs):
    import train
    from networks.unet import Encoder, Decoder
    from ramdsir import gpu_val
    from utils.metrics import post_and_dice, postprocess_binary
    os.makedirs(os.path.join(out_dir, 'host'), exist_ok=True)
    os.makedirs(os.path.join(out_dir, 'gpu'), exist_ok=True)
    host = train.start_host_val(data_dir, 0, bs)
    loader = host[0]
    ck = torch.load(ck_path, map_location='cpu')
    enc, dec = Encoder().cuda(), Decoder(num_classes=2).cuda()
    enc.load_state_dict(ck['encoder_state_dict'])
    dec.load_state_dict(ck['seg_decoder_state_dict'])
    before = {k: v.clone() for m in (enc, dec) for k, v in m.state_dict().items()}
    rng_before = (torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone())
    res = gpu_val.preload(train.fundus_testset(data_dir, 0), batch_size=bs)
    assert res is not None, '--gpu_val: the test set does not fit in device memory'
    ret_gpu = train.test_fundus_gpu(enc, dec, 3, res, 0, os.path.join(out_dir, 'gpu'), bs)
    untouched = all(torch.equal(v, before[k]) for m in (enc, dec) for k, v in m.state_dict().items())
    untouched = untouched and torch.equal(torch.get_rng_state(), rng_before[0]) and torch.equal(torch.cuda.get_rng_state(), rng_before[1])
    ret_host = train.test_fundus(enc, dec, 3, data_dir, 0, os.path.join(out_dir, 'host'), bs, host=host)
    # per image: the GPU path's masks and Dice, and the host path's computed step by step as test_fundus does
    keep = []
    dice_gpu = gpu_val.validate(enc, dec, res, bs, keep=keep)
    gpu_masks, gpu_posts = [], []
    for mask, out, recs in keep:
        mask, out = mask.cpu().numpy(), out.cpu().numpy()
        for r in list(recs)[:min(bs, len(res) - len(gpu_masks))]:
            gpu_masks.append(mask[r.off:r.off + 2 * r.h * r.w].reshape(2, r.h, r.w))
            gpu_posts.append(out[r.off:r.off + 2 * r.h * r.w].reshape(2, r.h, r.w))
    dice_host, same_mask, same_post, sizes = [], [], [], []
    enc.eval()
    dec.eval()
    i = 0
    with torch.no_grad():
        for data, target, target_orig, ids in loader:
            pred = torch.sigmoid(dec(enc(data.cuda())))
            pred = F.interpolate(pred, size=(target_orig.size(2), target_orig.size(3)), mode='bilinear')
            masks = (pred > 0.75).to(torch.uint8).cpu().numpy()
            tg = target_orig.to(torch.uint8).numpy()
            for k in range(masks.shape[0]):
                dice_host.append(list(post_and_dice((masks[k], tg[k]))))
                same_mask.append(bool(np.array_equal(masks[k], gpu_masks[i])))
                same_post.append(bool(np.array_equal(postprocess_binary(gpu_masks[i]), gpu_posts[i])))
                sizes.append(list(masks[k].shape[1:]))
                i += 1
    train.close_host_val(host)
    csv = [open(os.path.join(out_dir, d, '0_val_log.csv')).read() for d in ('host', 'gpu')]
    print('RESULT ' + json.dumps(dict(ret_host=ret_host, ret_gpu=ret_gpu, dice_host=dice_host, dice_gpu=[list(d) for d in dice_gpu],
                                      same_mask=same_mask, same_post=same_post, sizes=sizes, untouched=untouched, csv=csv,
                                      foreground=[float(m.mean()) for m in gpu_masks])))


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]))
