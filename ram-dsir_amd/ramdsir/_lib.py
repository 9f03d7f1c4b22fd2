"""ctypes binding of libramdsir_hip.so (include/ramdsir.h).  No fallback: if the HIP library is
missing or a call fails, this raises -- the product path never routes around the kernels."""
import ctypes as C
import functools
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RAMDSIR_DEBUG_LIB=1: the debug build (`make debug`), whose dispatch honours RD_* environment overrides (csrc/common.h
# rd_switch); the product library has none
LIB_PATH = os.path.join(_HERE, 'libramdsir_hip_dbg.so' if os.environ.get('RAMDSIR_DEBUG_LIB') == '1' else 'libramdsir_hip.so')

RD_F32, RD_BF16 = 0, 1
MAXG = 16
STAT_SLOTS = 64
STAT_SLOTS_FOLD = 8
FIN_OWNER = 1
FIN_MAX_G = 8          # groups a folded finalize may have (csrc/bn_fin.h)
SRC_RAW, SRC_AFF, SRC_AFFACT, SRC_POOL, SRC_UP, SRC_BNBWD = range(6)
DST_PLAIN, DST_POOL, DST_UPY, DST_NONE = range(4)

vp, fp, i32, i64, f32 = C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_float


class RdSrc(C.Structure):
    _fields_ = [('ptr', vp), ('ptr2', vp), ('scale', fp), ('shift', fp), ('q', fp), ('out', vp), ('mode', i32), ('C', i32),
                ('slope', f32), ('n_off', i32), ('g_fixed', i32), ('fin_flags', i32), ('fin', vp)]


class RdDst(C.Structure):
    _fields_ = [('g', vp), ('z', vp), ('scale', fp), ('shift', fp), ('bstats', fp), ('kind', i32), ('act', i32),
                ('accumulate', i32), ('Cd', i32), ('slope', f32), ('n_off', i32), ('g_fixed', i32), ('pad_', i32)]


class RdConv(C.Structure):
    _fields_ = [('src', RdSrc * 2), ('nsrc', i32), ('taps', i32), ('w', vp), ('bias', fp), ('CinPad', i32),
                ('CoutPad', i32), ('N', i32), ('H', i32), ('W', i32), ('Cin', i32), ('Cout', i32), ('G', i32),
                ('gstart', i32 * (MAXG + 1)), ('emode', i32), ('out', vp), ('stats', fp), ('dst', RdDst * 2),
                ('c_split', i32), ('cu_limit', i32), ('w_tap_rows', i32), ('stat_slots', i32)]


class RdWgrad(C.Structure):
    _fields_ = [('a', RdSrc * 2), ('na', i32), ('taps', i32), ('dz', RdSrc), ('N', i32), ('H', i32), ('W', i32),
                ('Cin', i32), ('Cout', i32), ('G', i32), ('gstart', i32 * (MAXG + 1)), ('partial', fp), ('dW', fp),
                ('beta', f32), ('cu_limit', i32)]


class RdRoute(C.Structure):
    """rd_route_t (include/ramdsir.h): one launch an entry point would make."""
    _fields_ = [('kernel', C.c_char_p), ('grid', i32 * 3), ('block', i32), ('lds', i32), ('iarg', i32 * 6), ('stores_sources', i32)]


class RdBnFwd(C.Structure):
    _fields_ = [('stats', fp), ('conv_bias', fp), ('scale', fp), ('shift', fp), ('mean', fp), ('invstd', fp), ('gamma', fp * MAXG),
                ('beta', fp * MAXG), ('running_mean', fp * MAXG), ('running_var', fp * MAXG),
                ('num_batches_tracked', vp * MAXG), ('count', f32 * MAXG), ('C', i32), ('G', i32), ('eps', f32),
                ('momentum', f32), ('training', i32), ('nslots', i32)]


class RdBnBwd(C.Structure):
    _fields_ = [('bstats', fp), ('mean', fp), ('invstd', fp), ('gamma', fp * MAXG), ('dgamma', fp * MAXG),
                ('dbeta', fp * MAXG), ('P', fp), ('Q', fp), ('R', fp), ('count', f32 * MAXG), ('C', i32), ('G', i32),
                ('fstats', fp), ('conv_bias', fp), ('dbias', fp), ('nslots', i32), ('pad_', i32)]


class RdSegLoss(C.Structure):
    _fields_ = [('logits', vp), ('target', vp), ('dlogits', vp), ('partial', fp), ('losses_out', fp), ('B', i32),
                ('H', i32), ('W', i32), ('K', i32), ('kind', i32), ('consistency', i32), ('cons_weight', f32),
                ('dlogits_cstride', i32)]


class RdAdam(C.Structure):
    _fields_ = [('param', fp), ('grad', fp), ('exp_avg', fp), ('exp_avg_sq', fp), ('n', i64), ('n_half_lr', i64),
                ('iter', vp), ('hyper_out', fp), ('base_lr', f32), ('total_iters', i32), ('beta1', f32),
                ('beta2', f32), ('eps', f32), ('pad_', i32)]


class RdRam(C.Structure):
    _fields_ = [('src', fp), ('trg', fp), ('lam', fp), ('out_img', vp), ('out_freq', vp), ('workspace', vp),
                ('tw_w', fp), ('tw_h', fp), ('B', i32), ('H', i32), ('W', i32), ('C', i32), ('b', i32),
                ('clip_lo', f32), ('clip_hi', f32), ('scale', f32), ('offset', f32), ('out_cstride', i32), ('src_u8', i32),
                ('div', f32), ('pad_', i32), ('trg_amp', fp), ('dft_tables', vp)]


class RdPackEntry(C.Structure):
    _fields_ = [('src_off', i64), ('dst_off', i64), ('start', i64), ('Cout', i32), ('Cin', i32), ('taps', i32),
                ('transpose', i32), ('RowPad', i32), ('ColPad', i32)]


AUG_CHUNK = 48         # RD_AUG_CHUNK


class RdAugImage(C.Structure):
    _fields_ = [('off', i64), ('mask_off', i64), ('h', i32), ('w', i32), ('tab_x', i32), ('tab_y', i32)]


class RdFundusSample(C.Structure):
    _fields_ = [('img', i32), ('partner', i32), ('tab_x', i32), ('tab_y', i32), ('sw', i32), ('sh', i32), ('cx', i32), ('cy', i32),
                ('lam', f32), ('pad_', i32)]


class RdFundusBatch(C.Structure):
    _fields_ = [('pixels', vp), ('masks', vp), ('images', vp), ('tables', vp), ('src', vp), ('trg', vp), ('lam', fp), ('mask', fp),
                ('n_images', i32), ('S', i32), ('id_x', i32), ('id_y', i32), ('band_rows', i32), ('src_rows', i32), ('mid_rows', i32),
                ('pad_', i32)]


class RdProstateSample(C.Structure):
    _fields_ = [('img', i32), ('partner', i32), ('lam', f32), ('pad_', i32)]


class RdProstateBatch(C.Structure):
    _fields_ = [('slices', fp), ('masks', vp), ('src', fp), ('trg', fp), ('lam', fp), ('mask', vp), ('n_slices', i32), ('S', i32)]


VAL_CHUNK = 32         # RD_VAL_CHUNK


class RdValImage(C.Structure):
    _fields_ = [('off', i64), ('gt_off', i64), ('h', i32), ('w', i32), ('slot', i32), ('pad_', i32)]


class RdValVolume(C.Structure):
    _fields_ = [('off', i64), ('gt_off', i64), ('d', i32), ('h', i32), ('w', i32), ('slot', i32)]


class RdBnEvalSite(C.Structure):
    """rd_bn_eval_site_t (include/ramdsir.h): one BatchNorm site of a frozen plan, a row of rd_bn_eval_coeffs' device table."""
    _fields_ = [('gamma', fp), ('beta', fp), ('running_mean', fp), ('running_var', fp), ('scale', fp), ('shift', fp), ('C', i32), ('pad_', i32)]


TB_F32, TB_BF16, TB_I64 = range(3)                                  # RD_TB_* element types
TB_IDENTITY, TB_SIGMOID, TB_TANH, TB_ARGMAX, TB_LABEL = range(5)      # RD_TB_* transforms
TB_MAX_GRIDS, TB_PALETTE = 8, 21


class RdTbGrid(C.Structure):
    _fields_ = [('src', vp), ('dst', vp), ('stride_n', i64), ('stride_c', i64), ('stride_h', i64), ('stride_w', i64), ('etype', i32),
                ('H', i32), ('W', i32), ('n', i32), ('sample', i32 * 3), ('c0', i32), ('nc', i32), ('transform', i32),
                ('normalize', i32), ('slot', i32)]


LOG_ROW, LOG_MAX_REC, LOG_CHUNK = 32, 16, 4096                      # RD_LOG_ROW, RD_LOG_MAX_REC, RD_LOG_CHUNK


class RdStepLog(C.Structure):
    """rd_step_log_t (include/ramdsir.h): one row of the per-step record ring."""
    _fields_ = [('losses', fp), ('rec_mse', fp), ('hyper', fp), ('grads', fp), ('range', i64 * 4), ('ring', fp), ('rows', i32), ('row', i32),
                ('n_rec', i32), ('pad_', i32), ('partial', vp)]


SNAP_CHUNK, SNAP_SUM_STRIDE = 65536, 16                             # RD_SNAP_CHUNK, RD_SNAP_SUM_STRIDE (64-bit words)


class RdSnapRange(C.Structure):
    """rd_snap_range_t (include/ramdsir.h): one range of rd_snapshot's table."""
    _fields_ = [('ptr', vp), ('bytes', i64), ('offset', i64), ('chunk0', i64)]


AVG_CHUNK = 16384                                                   # RD_AVG_CHUNK
AVG_F32, AVG_COPY = 0, 1                                            # rd_avg_range_t.kind
AVG_EMA, AVG_UNIFORM = 0, 1                                         # rd_avg_step's mode


class RdAvgRange(C.Structure):
    """rd_avg_range_t (include/ramdsir.h): one range pair of rd_avg_step's table."""
    _fields_ = [('src', vp), ('dst', vp), ('bytes', i64), ('chunk0', i64), ('kind', i32), ('pad_', i32)]


BN_RECAL_MAX_SITES = 4096                                           # RD_BN_RECAL_MAX_SITES


class RdBnRecalSite(C.Structure):
    """rd_bn_recal_site_t (include/ramdsir.h): one BatchNorm site of a recal plan, a row of rd_bn_recal's table."""
    _fields_ = [('stats', fp), ('conv_bias', fp), ('running_mean', fp), ('running_var', fp), ('num_batches_tracked', vp), ('count', f32),
                ('C', i32), ('nslots', i32), ('pad_', i32)]


GUARD_CHUNK = 16384                                                 # RD_GUARD_CHUNK
GUARD_MAX_N = 1 << 24                                               # elements rd_grad_guard accepts (rd_step_log's bound)


class RdGuardState(C.Structure):
    """rd_guard_state_t (include/ramdsir.h): the 40 device-resident bytes the guarded step's launches communicate through."""
    _fields_ = [('norm', f32), ('scale', f32), ('skip', i32), ('nonfinite', i32), ('steps', i64), ('clipped', i64), ('skipped', i64)]


class RdGradGuard(C.Structure):
    """rd_grad_guard_t (include/ramdsir.h): the descriptor of rd_grad_guard."""
    _fields_ = [('grad', fp), ('n', i64), ('max_norm', f32), ('pad_', i32), ('workspace', vp), ('state', vp)]


class RdGuardRange(C.Structure):
    """rd_guard_range_t (include/ramdsir.h): one live / shadow pair of rd_guard_sync's table."""
    _fields_ = [('live', vp), ('shadow', vp), ('bytes', i64), ('chunk0', i64)]


OPT_CHUNK = 4096                                                    # RD_OPT_CHUNK (elements)
OPT_MAX_RANGES = 4096                                               # RD_OPT_MAX_RANGES
OPT_POLY, OPT_COSINE, OPT_CONSTANT = 0, 1, 2                        # rd_optim_t.schedule
OPT_DECOUPLED, OPT_L2 = 0, 1                                        # rd_optim_t.wd_mode


class RdOptim(C.Structure):
    """rd_optim_t (include/ramdsir.h): the descriptor of rd_optim_step -- rd_adam_t without n_half_lr, with the schedule fields."""
    _fields_ = [('param', fp), ('grad', fp), ('exp_avg', fp), ('exp_avg_sq', fp), ('n', i64), ('iter', vp), ('hyper_out', fp),
                ('base_lr', f32), ('total_iters', i32), ('beta1', f32), ('beta2', f32), ('eps', f32), ('schedule', i32),
                ('warmup_iters', i32), ('wd_mode', i32)]


class RdOptimRange(C.Structure):
    """rd_optim_range_t (include/ramdsir.h): one param group of rd_optim_step's table, a contiguous range of the arena."""
    _fields_ = [('first', i64), ('count', i64), ('lr_mult', f32), ('weight_decay', f32), ('chunk0', i64)]


ACCUM_MAX_STEPS = 65536                                             # RD_ACCUM_MAX_STEPS

HIST_CHUNK = 16384                                                  # RD_HIST_CHUNK (elements)
HIST_MAX_LIMITS = 4096                                              # RD_HIST_MAX_LIMITS
HIST_MAX_RANGES = 4096                                              # RD_HIST_MAX_RANGES


class RdHistRange(C.Structure):
    """rd_hist_range_t (include/ramdsir.h): one tensor of rd_hist's table, an absolute device pointer and an element count."""
    _fields_ = [('src', vp), ('count', i64), ('chunk0', i64)]


class RdHistStats(C.Structure):
    """rd_hist_stats_t (include/ramdsir.h): the statistics record rd_hist writes per range."""
    _fields_ = [('min', C.c_double), ('max', C.c_double), ('sum', C.c_double), ('sum_squares', C.c_double), ('num', i64),
                ('nonfinite', i64)]


class RdLaunch(C.Structure):
    """rd_launch_t (include/ramdsir.h): one entry of a native launch list."""
    _fields_ = [('op', i32), ('lane', i32), ('wait_main', i32), ('nargs', i32), ('a', C.c_uint64 * 18)]


class RdStep(C.Structure):
    """rd_step_t (include/ramdsir.h): one step of rd_run_list_schedule."""
    _fields_ = [('kind', i32), ('lane', i32), ('index', i32), ('carries', i32)]


OP_FORK, OP_JOIN = 1, 2                              # RD_OP_FORK, RD_OP_JOIN
STEP_LAUNCH, STEP_FORK, STEP_JOIN = range(3)         # RD_STEP_*


@functools.lru_cache(maxsize=None)
def op_code(name):
    """The RD_OP_* code of an entry point, from the library's own table (include/ramdsir.h RD_LAUNCH_OPS)."""
    code = lib().rd_op_code(name.encode())
    if code < 0:
        raise KeyError('%s cannot go into a launch list' % name)
    return code


_SIGS = {
    'rd_ram_workspace': (i64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    'rd_ram_mix': (C.c_int, [C.POINTER(RdRam), C.c_int, vp]),
    'rd_ram_dft_tables_bytes': (i64, [C.c_int, C.c_int, C.c_int]),
    'rd_ram_dft_tables': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp]),
    'rd_ram_amp_workspace': (i64, [C.c_int, C.c_int, C.c_int]),
    'rd_ram_amp': (C.c_int, [fp, fp, C.c_int, C.c_int, C.c_int, vp, fp, fp, vp]),
    'rd_ram_mutate': (C.c_int, [fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, f32, vp]),
    'rd_pack_weights_batched': (C.c_int, [fp, vp, vp, C.c_int, i64, C.c_int, vp]),
    'rd_conv': (C.c_int, [C.POINTER(RdConv), C.c_int, vp]),
    'rd_wgrad_workspace': (i64, [C.POINTER(RdWgrad), C.c_int]),
    'rd_wgrad': (C.c_int, [C.POINTER(RdWgrad), C.c_int, vp]),
    'rd_wgrad_reduce': (C.c_int, [fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, f32, vp]),
    'rd_conv_honours_src_out': (C.c_int, [C.POINTER(RdConv), C.c_int]),
    'rd_conv_route': (C.c_int, [C.POINTER(RdConv), C.c_int, C.POINTER(RdRoute)]),
    'rd_wgrad_route': (C.c_int, [C.POINTER(RdWgrad), C.c_int, C.POINTER(RdRoute)]),
    'rd_conv_bwd_fused_route': (C.c_int, [C.POINTER(RdConv), C.POINTER(RdWgrad), C.c_int, C.POINTER(RdRoute)]),
    'rd_conv_bwd_fused_ok': (C.c_int, [C.POINTER(RdConv), C.POINTER(RdWgrad), C.c_int]),
    'rd_conv_bwd_fused_workspace': (i64, [C.POINTER(RdConv), C.POINTER(RdWgrad), C.c_int]),
    'rd_conv_bwd_fused': (C.c_int, [C.POINTER(RdConv), C.POINTER(RdWgrad), C.c_int, vp]),
    'rd_conv_bwd_fused_reduce': (C.c_int, [C.POINTER(RdConv), C.POINTER(RdWgrad), C.c_int, vp]),
    'rd_pack_weights': (C.c_int, [fp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    'rd_packed_elems': (i64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    'rd_bn_finalize_fwd': (C.c_int, [C.POINTER(RdBnFwd), vp]),
    'rd_bn_finalize_bwd': (C.c_int, [C.POINTER(RdBnBwd), vp]),
    'rd_gn_finalize_fwd': (C.c_int, [C.POINTER(RdBnFwd), vp]),
    'rd_gn_finalize_bwd': (C.c_int, [C.POINTER(RdBnBwd), vp]),
    'rd_bn_apply': (C.c_int, [vp, vp, vp, fp, fp, fp, f32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(i32), C.c_int, vp]),
    'rd_up_stats': (C.c_int, [vp, fp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(i32), C.c_int, C.c_int, vp]),
    'rd_bn_stats': (C.c_int, [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(i32), C.c_int, vp]),
    'rd_pool_fwd': (C.c_int, [vp, fp, fp, f32, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(i32), C.c_int, vp, C.c_int, vp]),
    'rd_pool_bwd': (C.c_int, [vp, vp, fp, fp, f32, C.c_int, vp, C.c_int, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(i32), C.c_int, C.c_int, vp]),
    'rd_up_bwd': (C.c_int, [vp, vp, vp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(i32),
                            C.c_int, vp, C.c_int, vp]),
    'rd_nchw_to_nhwc': (C.c_int, [fp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    'rd_nhwc_to_nchw': (C.c_int, [vp, fp, fp, fp, C.c_int, f32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.POINTER(i32), C.c_int, vp]),
    'rd_grad_in': (C.c_int, [fp, vp, vp, fp, fp, fp, C.c_int, f32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                             C.c_int, C.POINTER(i32), C.c_int, vp]),
    'rd_colsum': (C.c_int, [vp, fp, fp, i64, C.c_int, C.c_int, f32, C.c_int, vp]),
    'rd_seg_loss_workspace': (i64, [C.POINTER(RdSegLoss)]),
    'rd_seg_loss': (C.c_int, [C.POINTER(RdSegLoss), C.c_int, vp]),
    'rd_rec_loss': (C.c_int, [vp, vp, vp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(i32), f32,
                              C.c_int, vp]),
    'rd_rec_loss_workspace': (i64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    'rd_adam_step': (C.c_int, [C.POINTER(RdAdam), vp]),
    'rd_zero': (C.c_int, [C.POINTER(vp), C.POINTER(i64), C.c_int, vp]),
    'rd_run_list': (C.c_int, [C.POINTER(RdLaunch), C.c_int, C.POINTER(vp), C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    'rd_join_lanes': (C.c_int, [C.POINTER(vp), C.c_int, C.c_uint32]),
    'rd_run_list_threads': (C.c_int, [C.c_int]),
    'rd_run_list_bind_fork_events': (C.c_int, [C.c_int]),
    'rd_run_list_fork_counts': (None, [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    'rd_run_list_fork_plan': (C.c_int, [C.POINTER(RdLaunch), C.c_int, C.POINTER(C.c_ubyte)]),
    'rd_run_list_schedule': (C.c_int, [C.POINTER(RdLaunch), C.c_int, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(RdStep),
                                       C.POINTER(C.c_int)]),
    'rd_op_code': (C.c_int, [C.c_char_p]),
    'rd_tb_grids_workspace': (i64, [C.c_int]),
    'rd_tb_grids': (C.c_int, [C.POINTER(RdTbGrid), C.c_int, vp, i64, vp]),
    'rd_step_log': (C.c_int, [C.POINTER(RdStepLog), vp]),
    'rd_step_log_workspace': (i64, [i64]),
    'rd_snapshot': (C.c_int, [C.POINTER(RdSnapRange), vp, C.c_int, i64, vp, i64, vp, C.c_int, vp]),
    'rd_avg_step': (C.c_int, [C.POINTER(RdAvgRange), vp, C.c_int, i64, vp, C.c_int, f32, i32, vp]),
    'rd_bn_recal': (C.c_int, [C.POINTER(RdBnRecalSite), vp, C.c_int, C.c_int, i32, f32, vp]),
    'rd_grad_guard_workspace': (i64, [i64]),
    'rd_grad_guard': (C.c_int, [C.POINTER(RdGradGuard), vp]),
    'rd_adam_step_guarded': (C.c_int, [C.POINTER(RdAdam), vp, vp]),
    'rd_guard_sync': (C.c_int, [C.POINTER(RdGuardRange), vp, C.c_int, i64, vp, vp]),
    'rd_optim_step': (C.c_int, [C.POINTER(RdOptim), C.POINTER(RdOptimRange), vp, C.c_int, i64, vp, vp]),
    'rd_grad_accum': (C.c_int, [fp, fp, i64, i32, i32, f32, vp]),
    'rd_hist_workspace': (i64, [i64]),
    'rd_hist': (C.c_int, [C.POINTER(RdHistRange), vp, C.c_int, i64, vp, vp, C.c_int, vp, vp, vp, vp]),
    'rd_crc32c':(C.c_uint32, [vp, C.c_size_t, C.c_uint32]),
    'rd_box_probe': (C.c_int, [C.c_int, vp, vp, i64, vp]),
    'rd_fundus_batch': (C.c_int, [C.POINTER(RdFundusBatch), C.POINTER(RdFundusSample), C.c_int, vp]),
    'rd_prostate_batch': (C.c_int, [C.POINTER(RdProstateBatch), C.POINTER(RdProstateSample), C.c_int, vp]),
    'rd_val_threshold': (C.c_int, [fp, C.c_int, C.c_int, C.c_int, C.POINTER(RdValImage), vp, i64, vp]),
    'rd_val_post_workspace': (i64, [C.POINTER(RdValImage), C.c_int]),
    'rd_val_post': (C.c_int, [vp, vp, i64, vp, i64, vp, C.c_int, vp, i64, C.POINTER(RdValImage), C.c_int, vp]),
    'rd_vol_stack': (C.c_int, [fp, C.c_int, C.c_int, C.c_int, C.POINTER(i32), C.c_int, fp, vp]),
    'rd_vol_argmax': (C.c_int, [fp, C.c_int, C.c_int, C.c_int, C.POINTER(i32), vp, C.c_int, vp, vp]),
    'rd_vol_post_workspace': (i64, [C.POINTER(RdValVolume), C.c_int]),
    'rd_vol_post': (C.c_int, [vp, vp, i64, vp, i64, vp, C.c_int, vp, i64, C.POINTER(RdValVolume), C.c_int, vp]),
    'rd_bn_eval_coeffs': (C.c_int, [vp, C.c_int, C.c_int, f32, vp]),
    'rd_val_threshold_nhwc': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(RdValImage), vp, i64, vp]),
    'rd_vol_stack_nhwc': (C.c_int, [fp, C.c_int, C.c_int, C.c_int, C.POINTER(i32), C.c_int, vp, C.c_int, C.c_int, vp]),
    'rd_vol_argmax_nhwc': (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(i32), vp, C.c_int, vp, vp]),
}

_lib = None


def exported_symbols():
    return sorted(_SIGS)


def lib():
    """The loaded library (cached).  Raises if it has not been built (run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError('libramdsir_hip.so is not built: run `make -C ram-dsir_amd/csrc` '
                               '(or __graft_entry__.build()); there is no CPU fallback')
        # ONE HIP runtime per process: the library's libamdhip64.so.7 must be the copy PyTorch ships and has initialised (the streams and
        # device pointers handed to the entry points are that runtime's).  Loaded before torch, the dynamic linker would bind it to
        # /opt/rocm/lib's copy and the first launch on a torch stream fails with hipErrorNoDevice (__graft_entry__.build() followed by
        # smoke() in one process did) -- so torch comes first, whatever the caller's import order.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(err, what=''):
    if err != 0:
        raise RuntimeError('ramdsir HIP call failed (%s): error %d' % (what, err))


def pack_arg(value, ctype):
    """One argument of an entry point as the 64-bit word rd_launch_t.a[] carries (include/ramdsir.h): pointers and integers as they
    are, a float as its bit pattern."""
    import struct
    if value is None:
        return 0
    if ctype is f32 or ctype is C.c_float:
        return struct.unpack('<I', struct.pack('<f', float(value)))[0]
    if ctype in (C.c_int, i32, i64, C.c_int64, C.c_uint32):
        return int(value) & 0xFFFFFFFFFFFFFFFF
    # pointer-like: byref(obj), a ctypes array / structure, a c_void_p, or a raw address
    if hasattr(value, '_obj'):
        return C.addressof(value._obj)
    if isinstance(value, (C.Array, C.Structure)):
        return C.addressof(value)
    if isinstance(value, C.c_void_p):
        return value.value or 0
    return int(value)


def gstart_array(gs):
    a = (i32 * (MAXG + 1))()
    for i, v in enumerate(gs):
        a[i] = int(v)
    return a


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    """torch's current stream as the c_void_p that every entry point declares for its trailing stream argument."""
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
