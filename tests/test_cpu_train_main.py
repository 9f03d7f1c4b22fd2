"""CPU-only tests of train.py's stages: the flag sets check_args refuses (directly and through main(), which must stop before
any GPU call), the validation mode as a function of the flags and of what is on disk / fits, and the reference's CSV lines
(code/train.py:124-132, 186-192) byte for byte.  No GPU call is made and the HIP library is not loaded."""
import pytest
import torch

import train

BASE = ['--save_path', 'unused', '--ram', '--rec', '--data_root', '/nonexistent']
CKPT_FLAGS = [['--ckpt_every', '1'], ['--resume', 'f.pth'], ['--ckpt_every', '1', '--stop_after_epochs', '1']]

# (flags behind --save_path, WORLD_SIZE, a substring of the refusal)
REFUSED = [
    (['--save_path', 'unused'], 1, 'only the --ram --rec flag combination'),
    (['--save_path', 'unused', '--ram'], 1, 'ram=True rec=False'),
    (BASE + ['--gpu_val', '--dataset', 'prostate'], 1, '--gpu_val covers the in-training Fundus validation only'),
    (BASE + ['--gpu_val_volumes'], 1, '--gpu_val_volumes covers the in-training Prostate validation only'),
    (BASE + ['--fused_val'], 1, 'it needs --gpu_val (fundus) or --gpu_val_volumes (prostate)'),
    (BASE + ['--fused_val', '--gpu_val', '--norm', 'gn'], 1, '--fused_val freezes BatchNorm on its running statistics: --norm gn'),
    (BASE + ['--tb_images', '-3'], 1, '--tb_images takes a positive interval, got -3'),
    (BASE + ['--tb_every_iter', '--norm', 'in'], 1, "read the fused step's device buffers: --norm in"),
    (BASE + ['--tb_health', '--norm', 'in'], 1, "read the fused step's device buffers: --norm in"),
    (BASE + ['--ckpt_every', '-1'], 1, 'take a number of epochs, got -1 / 0'),
    (BASE + ['--stop_after_epochs', '2'], 1, 'it needs --ckpt_every'),
] + [(BASE + f + ['--norm', 'gn'], 1, "snapshot the fused step's arenas: --norm gn") for f in CKPT_FLAGS] \
  + [(BASE + f, 2, 'run in one process') for f in CKPT_FLAGS]


@pytest.mark.parametrize('argv,world,message', REFUSED)
def test_check_args_refuses_and_main_stops_there(argv, world, message, monkeypatch):
    args = train.parse_args(argv)
    with pytest.raises(ValueError) as e:
        train.check_args(args, world)
    assert message in str(e.value)
    monkeypatch.setenv('WORLD_SIZE', str(world))
    with pytest.raises(ValueError) as e:                    # --resume f.pth does not exist: the refusal comes before the file is opened
        train.main(train.parse_args(argv))
    assert message in str(e.value)
    assert not torch.cuda.is_initialized()


def test_check_args_accepts_what_the_runs_use():
    for extra in ([], ['--gpu_data', '--gpu_val', '--fused_val', '--tb_images', '2', '--tb_every_iter', '--tb_health', '--ckpt_every', '1'],
                  ['--dataset', 'prostate', '--gpu_data', '--gpu_val_volumes', '--fused_val'], ['--norm', 'gn']):
        assert train.check_args(train.parse_args(BASE + extra), 1) is None
    assert train.check_args(train.parse_args(BASE), 8) is None


NOT_IN_USE = 'fused_val: the resident validation is not in use: validating through the modules'
NOT_TWO = 'gpu_val_volumes: --num_classes 3 is not 2: validating on the host'
PROSTATE = ['--dataset', 'prostate', '--num_classes', '2']

# (flags, data on disk, resident preload fits, (mode, line at the preload, line at the bind))
MODES = [
    ([], False, True, ('none', None, None)),
    ([], True, True, ('host', None, None)),
    (['--gpu_val'], True, True, ('resident', None, None)),
    (['--gpu_val'], True, False, ('host', None, None)),
    (['--gpu_val', '--fused_val'], True, True, ('fused', None, None)),
    (['--gpu_val', '--fused_val'], True, False, ('host', None, NOT_IN_USE)),
    (['--gpu_val', '--fused_val'], False, True, ('none', None, NOT_IN_USE)),
    (['--dataset', 'prostate', '--num_classes', '3', '--gpu_val_volumes'], True, True, ('host', NOT_TWO, None)),
    (['--dataset', 'prostate', '--num_classes', '3', '--gpu_val_volumes', '--fused_val'], True, True, ('host', NOT_TWO, NOT_IN_USE)),
    (PROSTATE + ['--gpu_val_volumes'], True, True, ('resident', None, None)),
    (PROSTATE + ['--gpu_val_volumes'], True, False, ('host', None, None)),
    (PROSTATE + ['--gpu_val_volumes', '--fused_val'], True, True, ('fused', None, None)),
    (PROSTATE, True, True, ('host', None, None)),
    (PROSTATE + ['--gpu_val_volumes'], False, True, ('none', None, None)),
    (PROSTATE, False, True, ('none', None, None)),
]


@pytest.mark.parametrize('flags,on_disk,fits,want', MODES)
def test_val_mode(flags, on_disk, fits, want):
    assert tuple(train.val_mode(train.parse_args(BASE + flags), on_disk, fits)) == want


def test_validation_object_finds_nothing_on_disk_and_starts_nothing(tmp_path):
    """Data absent: no loader, no pool, no draw from torch's generator, and the per-epoch call has nothing to do."""
    for flags in ([], ['--gpu_val'], PROSTATE + ['--gpu_val_volumes']):
        args = train.parse_args(['--save_path', str(tmp_path), '--ram', '--rec'] + flags)
        before = torch.get_rng_state()
        val = train.Validation(args, str(tmp_path / args.dataset))
        assert (val.on_disk, val.mode, val.host, val.resident, val.forward) == (False, 'none', None, None, None)
        assert val(None, None, 0) is None
        val.close()
        assert torch.equal(torch.get_rng_state(), before)
    assert not torch.cuda.is_initialized()


def test_gpu_val_takes_the_one_draw_of_the_loader_it_does_not_start(tmp_path):
    """Data present with --gpu_val: the constructor takes exactly the 64-bit draw a DataLoader iterator takes for its base seed."""
    root = tmp_path / 'fundus'
    root.mkdir()
    (root / 'Domain1_test.list').write_text('')
    args = train.parse_args(['--save_path', str(tmp_path), '--ram', '--rec', '--gpu_val', '--test_domain_idx', '0'])
    torch.manual_seed(7)
    val = train.Validation(args, str(root))
    after = torch.get_rng_state()
    assert (val.on_disk, val.mode, val.host) == (True, 'resident', None)
    torch.manual_seed(7)
    torch.empty((), dtype=torch.int64).random_()
    assert torch.equal(torch.get_rng_state(), after)
    assert not torch.cuda.is_initialized()


def test_csv_lines_are_the_references(tmp_path, capsys):
    ret = train.report_fundus([(0.5, 0.25)], 3, 2, str(tmp_path), 8)
    assert ret == (0.5 + 0.25) * 100 / 2
    assert (tmp_path / '2_val_log.csv').read_text() == "['batch-size: ', 8, 3, 'cup dice coefficence: ', 0.5, 'disc dice coefficence: ', 0.25]\n"
    ret = train.report_prostate(0.75, 3, 4, str(tmp_path), 8)
    assert ret == 0.75 * 100
    assert (tmp_path / '4_val_log.csv').read_text() == "['batch-size: ', 8, 3, 'dice coefficence: ', 0.75]\n"
    assert capsys.readouterr().out == 'val_cup_dice : 0.5, val_disc_dice : 0.25\nval_dice : 0.75\n'
    # the file is appended to, and the mean is taken over the images in list order
    assert train.report_fundus([(1.0, 0.5), (0.5, 0.0)], 4, 2, str(tmp_path), 8) == (0.75 + 0.25) * 100 / 2
    assert (tmp_path / '2_val_log.csv').read_text().splitlines()[1] == \
        "['batch-size: ', 8, 4, 'cup dice coefficence: ', 0.75, 'disc dice coefficence: ', 0.25]"
    assert train.report_fundus([], 5, 2, str(tmp_path), 8) == 0.0                  # an empty test list: 0 / max(0, 1)
