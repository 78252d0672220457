"""What the trainer's C boundary answers to a bad call: (return code, gmz_last_error() text) of every check between
GMZ_EXPORT and the first launch in csrc/gmz_train.hip, gmz_heads.hip and gmz_conv.hip, held byte for byte to
tests/golden/abi_messages.json (recorded by tests/golden/make_golden_abi_messages.py from the build BEFORE the host
code of those files was folded, and not regenerated since: callers and tests match on these texts).

Each case is an otherwise valid argument list with one thing wrong, so it stops at one particular check: the checks of
every exported function of the three files and of the host helpers they call (check_layout, check_bn_ws, check_parts,
check_slots, head_check, bad_size, the "relu_mask needs ..." refusal of the BatchNorm launchers, launch_conv3's "A/B
variants are built for 9 and 15 only"), and the bad-dtype answer of every entry point that takes a dtype (the last
check before the dispatch).  The pointers are fake (1 << 20, 16-B aligned; + 4 where a case is about alignment) and
never dereferenced; the valid baseline itself is never called.

Not covered, because no argument alone reaches them (they need a HIP call's result):
  "hipGetLastError(): <HIP error text> @<file>:<line>"   GMZ_LAUNCH_CHECK after every launch of the three files (the
                                                          only GMZ_HIP sites there): needs a launch to have failed

A recorded text of that shape would mean a case got past validation and launched on a fake pointer: the generator
refuses to record one and the test asserts none is in the fixture.  For the same reason the module is for machines
without a GPU (there the launch cannot happen) and skips itself on one.
"""
import ctypes
import json
import os
import re

import pytest
import torch

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "abi_messages.json")

FAKE = 1 << 20


def p(k):
    """Fake, 16-B aligned, pairwise distinct device pointers."""
    return FAKE + 4096 * k


ODD = FAKE + 4  # 4-B aligned only

# GMZ_HIP's message: the stringified call, a colon, HIP's text, " @" + the source file + ":" + the line
_HIP_TAIL = re.compile(r" @\S*\.(?:hip|h):\d+$")
_HIP_HEAD = re.compile(r"^\(?\s*hip[A-Z]\w*\s*\(")


def got_past_validation(text):
    return bool(_HIP_TAIL.search(text) or _HIP_HEAD.search(text))


def _query(lib, name, *args, ctype=ctypes.c_size_t):
    out = ctype()
    assert getattr(lib, name)(*args, ctypes.byref(out)) == 0, name
    return out.value


def build_cases(lib):
    """[(case id, function name, argument tuple)]: per entry point a valid baseline and cases that change it."""
    cases = []
    base = {}

    def entry(fn, **valid):
        base[fn] = valid

    def bad(fn, what, **wrong):
        assert wrong and not set(wrong) - set(base[fn]), (fn, what)  # never the valid baseline itself
        args = dict(base[fn], **wrong)
        cases.append(("%s/%s" % (fn, what), fn, tuple(args.values())))

    # ------------------------------------------------------------------ gmz_train.hip: optimiser, clock, gradients
    item_b, chunk, opt_ws = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
    assert lib.gmz_opt_layout(ctypes.byref(item_b), ctypes.byref(chunk), ctypes.byref(opt_ws)) == 0
    entry("gmz_opt_layout", item_bytes=ctypes.byref(item_b), chunk=ctypes.byref(chunk), ws=ctypes.byref(opt_ws))
    bad("gmz_opt_layout", "null", chunk=None)
    entry("gmz_opt_step", items=p(1), n_items=4, grad=p(2), exp_avg=p(3), exp_avg_sq=p(4), n=1000, scale=None,
          skip_on_inf=1, max_norm=5.0, lr=p(5), beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-5, tau=0.995, step=p(6),
          coef=p(7), ws=p(8), ws_bytes=opt_ws.value, stream=None)
    bad("gmz_opt_step", "null", lr=None)
    bad("gmz_opt_step", "n_items", n_items=0)
    bad("gmz_opt_step", "workspace", ws_bytes=opt_ws.value - 1)
    bad("gmz_opt_step", "aligned", grad=ODD)
    entry("gmz_comm_stamp", acc=p(1), phase=0, stream=None)
    bad("gmz_comm_stamp", "null", acc=None)
    bad("gmz_comm_stamp", "phase", phase=3)
    entry("gmz_grad_add_t_cols", dtype=1, src=p(1), P=9, C=16, O=8, ldo=12, col0=4, dst=p(2), stream=None)
    bad("gmz_grad_add_t_cols", "null", dst=None)
    bad("gmz_grad_add_t_cols", "ldo", ldo=11)
    bad("gmz_grad_add_t_cols", "too_large", P=1 << 15, C=1 << 10, ldo=1 << 6, O=8, col0=0)
    bad("gmz_grad_add_t_cols", "grid_z", P=1, C=65536, O=1, ldo=1, col0=0)
    bad("gmz_grad_add_t_cols", "dtype", dtype=7)
    entry("gmz_grad_add_t", dtype=1, src=p(1), P=9, C=16, O=8, dst=p(2), stream=None)
    bad("gmz_grad_add_t", "O", O=0)
    bad("gmz_grad_add_t", "grid_z", P=1, C=65536, O=1)
    bad("gmz_grad_add_t", "dtype", dtype=7)

    # ------------------------------------------------------------------ gmz_train.hip: BatchNorm
    B, C, S = 8, 16, 9
    need = ctypes.c_size_t()
    entry("gmz_bn_workspace_bytes", layout=1, B=B, C=C, S=S, out=ctypes.byref(need))
    bad("gmz_bn_workspace_bytes", "shape", S=0)
    bad("gmz_bn_workspace_bytes", "null", out=None)
    bad("gmz_bn_workspace_bytes", "layout", layout=2)
    bad("gmz_bn_workspace_bytes", "layout_odd_C", C=15)
    bad("gmz_bn_workspace_bytes", "layout_wide_C", C=514)
    ws1 = _query(lib, "gmz_bn_workspace_bytes", 1, B, C, S)  # channels-last
    ws0 = _query(lib, "gmz_bn_workspace_bytes", 0, B, C, S)
    ns = 4
    parts = C * ns * 24  # f64 [C][ns][3]
    huge = dict(B=1 << 11, C=1 << 10, S=1 << 10)  # B * C * S = 2^31

    fwd = dict(dtype=1, layout=1, x=p(1), res=None, mask=None, B=B, C=C, S=S, gamma=p(2), beta=p(3), eps=1e-4,
               momentum=0.1, rm=None, rv=None, nb=None, relu=1, y=p(4), save=p(5), ws=p(6), ws_bytes=ws1)
    entry("gmz_bn_forward", **fwd, stream=None)
    entry("gmz_bn_forward_m", **fwd, relu_mask=p(7), stream=None)
    for fn in ("gmz_bn_forward", "gmz_bn_forward_m"):
        bad(fn, "shape", B=0)
        bad(fn, "shape_2^31", **huge)
        bad(fn, "layout", layout=2)
        bad(fn, "layout_odd_C", C=15)
        bad(fn, "null", save=None)
        bad(fn, "workspace", ws_bytes=ws1 - 8)
        bad(fn, "workspace_nchw", layout=0, ws_bytes=ws0 - 8)
        bad(fn, "running_pair", rm=p(8))
        bad(fn, "dtype", dtype=7)
    bad("gmz_bn_forward_m", "relu_mask_no_relu", relu=0)
    bad("gmz_bn_forward_m", "relu_mask_nchw", layout=0, ws_bytes=ws0)
    bad("gmz_bn_forward_m", "relu_mask_unaligned", x=ODD)

    bwd = dict(dtype=1, layout=1, x=p(1), y=p(2), dy=p(3), mask=None, B=B, C=C, S=S, gamma=p(4), save=p(5), relu=1,
               dx=p(6), dres=None, dgamma=p(7), dbeta=p(8), ws=p(9), ws_bytes=ws1)
    entry("gmz_bn_backward", **bwd, stream=None)
    entry("gmz_bn_backward_acc", **bwd, stream=None, accumulate=1)
    entry("gmz_bn_backward_acc_m", **bwd, relu_mask=p(10), stream=None, accumulate=1)
    for fn in ("gmz_bn_backward", "gmz_bn_backward_acc", "gmz_bn_backward_acc_m"):
        bad(fn, "shape", C=0)
        bad(fn, "shape_2^31", **huge)
        bad(fn, "layout", layout=3)
        bad(fn, "null", dgamma=None)
        bad(fn, "null_y_with_relu", y=None)
        bad(fn, "workspace", ws_bytes=ws1 - 8)
        bad(fn, "dtype", dtype=7)
    bad("gmz_bn_backward_acc_m", "relu_mask_no_relu", relu=0)
    bad("gmz_bn_backward_acc_m", "relu_mask_nchw", layout=0, ws_bytes=ws0)
    bad("gmz_bn_backward_acc_m", "relu_mask_C", C=18, ws_bytes=_query(lib, "gmz_bn_workspace_bytes", 1, B, 18, S))

    fst = dict(dtype=1, x=p(1), res=None, B=B, C=C, S=S, gamma=p(2), beta=p(3), eps=1e-4, momentum=0.1, rm=None,
               rv=None, nb=None, relu=1, y=p(4), save=p(5), stats=p(6), ns=ns, stats_bytes=parts)
    entry("gmz_bn_forward_stats", **fst, stream=None)
    entry("gmz_bn_forward_stats_m", **fst, relu_mask=p(7), stream=None)
    for fn in ("gmz_bn_forward_stats", "gmz_bn_forward_stats_m"):
        bad(fn, "shape", S=-1)
        bad(fn, "shape_ns", ns=0)
        bad(fn, "shape_2^31", **huge)
        bad(fn, "layout_odd_C", C=15)
        bad(fn, "null", stats=None)
        bad(fn, "partials", stats_bytes=parts - 8)
        bad(fn, "running_pair", rv=p(8))
        bad(fn, "dtype", dtype=7)
    bad("gmz_bn_forward_stats_m", "relu_mask_no_relu", relu=0)
    bad("gmz_bn_forward_stats_m", "relu_mask_unaligned", y=ODD)

    entry("gmz_bn_forward_seg", dtype=1, x=p(1), res=None, mask=None, B=B, nseg=2, C=C, S=S, gamma=p(2), beta=p(3),
          eps=1e-4, momentum=0.1, rm=None, rv=None, nb=None, relu=1, y=p(4), save=p(5), ws=p(6), ws_bytes=ws1,
          board_stats=None, board_stats_bytes=0, stream=None)
    bad("gmz_bn_forward_seg", "shape", B=0)
    bad("gmz_bn_forward_seg", "shape_nseg", nseg=3)
    bad("gmz_bn_forward_seg", "shape_2^31", **huge)
    bad("gmz_bn_forward_seg", "layout_odd_C", C=15)
    bad("gmz_bn_forward_seg", "null", ws=None)
    bad("gmz_bn_forward_seg", "workspace", ws_bytes=ws1 - 8)
    # segments of fewer than 16 pixels: one partial slot each, more than gmz_bn_workspace_bytes asks for
    bad("gmz_bn_forward_seg", "workspace_tiny_segments", B=6, nseg=6, C=8, S=9,
        ws_bytes=_query(lib, "gmz_bn_workspace_bytes", 1, 6, 8, 9))
    bad("gmz_bn_forward_seg", "board_partials", board_stats=p(7), board_stats_bytes=C * B * 24 - 8)
    bad("gmz_bn_forward_seg", "running_pair", rm=p(8))
    bad("gmz_bn_forward_seg", "dtype", dtype=7)

    entry("gmz_bn_eval", dtype=1, layout=1, x=p(1), res=None, B=B, C=C, S=S, gamma=p(2), beta=p(3), rm=p(4), rv=p(5),
          eps=1e-4, relu=1, y=p(6), ws=p(7), ws_bytes=ws1, stream=None)
    bad("gmz_bn_eval", "shape", B=-2)
    bad("gmz_bn_eval", "shape_2^31", **huge)
    bad("gmz_bn_eval", "layout", layout=-1)
    bad("gmz_bn_eval", "null", rv=None)
    bad("gmz_bn_eval", "workspace", ws_bytes=ws1 - 8)
    bad("gmz_bn_eval", "dtype", dtype=7)

    entry("gmz_bn_backward_stats", dtype=1, x=p(1), y=p(2), dy=p(3), mask=None, B=B, C=C, S=S, gamma=p(4), save=p(5),
          relu=1, dx=p(6), dres=None, dgamma=p(7), dbeta=p(8), stats=p(9), ns=ns, stats_bytes=parts, ws=p(10),
          ws_bytes=ws1, stream=None, accumulate=0)
    bad("gmz_bn_backward_stats", "shape", B=0)
    bad("gmz_bn_backward_stats", "shape_ns", ns=-1)
    bad("gmz_bn_backward_stats", "shape_2^31", **huge)
    bad("gmz_bn_backward_stats", "layout_odd_C", C=15)
    bad("gmz_bn_backward_stats", "null", stats=None)
    bad("gmz_bn_backward_stats", "null_y_with_relu", y=None)
    bad("gmz_bn_backward_stats", "partials", stats_bytes=parts - 8)
    bad("gmz_bn_backward_stats", "workspace", ws_bytes=ws1 - 8)
    bad("gmz_bn_backward_stats", "partials_before_workspace", stats_bytes=parts - 8, ws_bytes=ws1 - 8)
    bad("gmz_bn_backward_stats", "dtype", dtype=7)

    entry("gmz_bn_forward_deferred", dtype=1, x=p(1), mask=None, B=B, C=C, S=S, eps=1e-4, momentum=0.1, rm=None,
          rv=None, nb=None, save=p(2), stats=p(3), ns=ns, stats_bytes=parts, ws=None, ws_bytes=0, stream=None)
    bad("gmz_bn_forward_deferred", "shape", C=0)
    bad("gmz_bn_forward_deferred", "shape_2^31", **huge)
    bad("gmz_bn_forward_deferred", "layout_odd_C", C=15)
    bad("gmz_bn_forward_deferred", "null", save=None)
    bad("gmz_bn_forward_deferred", "null_without_stats", stats=None, ns=0, stats_bytes=0)
    bad("gmz_bn_forward_deferred", "ns", ns=0)
    bad("gmz_bn_forward_deferred", "partials", stats_bytes=parts - 8)
    bad("gmz_bn_forward_deferred", "workspace", stats=None, ns=0, stats_bytes=0, ws=p(4), ws_bytes=ws1 - 8)
    bad("gmz_bn_forward_deferred", "running_pair", rm=p(8))
    bad("gmz_bn_forward_deferred", "dtype", dtype=7)
    bad("gmz_bn_forward_deferred", "dtype_without_stats", dtype=7, stats=None, ns=0, stats_bytes=0, ws=p(4),
        ws_bytes=ws1)

    # ------------------------------------------------------------------ gmz_heads.hip
    P = 81
    entry("gmz_head_conv1x1_workspace_bytes", P=P, O=3, out=ctypes.byref(need))
    bad("gmz_head_conv1x1_workspace_bytes", "P", P=0)
    bad("gmz_head_conv1x1_workspace_bytes", "O", O=5)
    bad("gmz_head_conv1x1_workspace_bytes", "null", out=None)
    head_ws = _query(lib, "gmz_head_conv1x1_workspace_bytes", P, 3)
    entry("gmz_head_conv1x1_forward", dtype=1, x=p(1), P=P, C=128, w0=p(2), b0=p(3), O0=2, w1=p(4), b1=p(5), O1=1,
          y0=p(6), y1=p(7), stream=None)
    entry("gmz_head_conv1x1_backward", dtype=1, x=p(1), P=P, C=128, w0=p(2), O0=2, w1=p(3), O1=1, dy0=p(4), dy1=p(5),
          dx=p(6), dw0=None, db0=None, dw1=None, db1=None, accumulate=0, ws=p(7), ws_bytes=head_ws, stream=None)
    for fn in ("gmz_head_conv1x1_forward", "gmz_head_conv1x1_backward"):
        bad(fn, "C", C=64)
        bad(fn, "P", P=0)
        bad(fn, "P_2^31", P=1 << 24)
        bad(fn, "O0", O0=0)
        bad(fn, "O_sum", O0=3, O1=2)
        bad(fn, "null", w0=None)
        bad(fn, "null_w1", w1=None)
        bad(fn, "x_unaligned", x=ODD)
        bad(fn, "dtype", dtype=7)
    bad("gmz_head_conv1x1_forward", "null_output", y0=None)
    bad("gmz_head_conv1x1_forward", "null_output_y1", y1=None)
    bad("gmz_head_conv1x1_backward", "null_operand", dx=None)
    bad("gmz_head_conv1x1_backward", "null_operand_dy1", dy1=None)
    bad("gmz_head_conv1x1_backward", "workspace", ws_bytes=head_ws - 4)
    bad("gmz_head_conv1x1_backward", "dx_unaligned", dx=ODD)

    entry("gmz_seg_bn_small_workspace_bytes", nseg=5, C=2, out=ctypes.byref(need))
    bad("gmz_seg_bn_small_workspace_bytes", "nseg", nseg=33)
    bad("gmz_seg_bn_small_workspace_bytes", "C", C=9)
    bad("gmz_seg_bn_small_workspace_bytes", "null", out=None)
    nseg, sB, sS, sC = 5, 8, 9, 2
    sbs_ws = _query(lib, "gmz_seg_bn_small_workspace_bytes", nseg, sC)
    st_b = 4 * (3 * nseg * sC + nseg)
    sfw = dict(dtype=1, x=p(1), row_mask=None, nseg=nseg, B=sB, S=sS, C=sC, gamma=p(2), beta=p(3), eps=1e-4, y=p(4),
               stats=p(5), stats_bytes=st_b, update=0, momentum=0.1, rm=None, rv=None, nb=None, pre_stats=None)
    entry("gmz_seg_bn_forward", **sfw, stream=None)
    entry("gmz_seg_bn_forward_small", **sfw, ws=p(6), ws_bytes=sbs_ws, stream=None)
    sbw = dict(dtype=1, x=p(1), dy=p(2), row_mask=None, nseg=nseg, B=sB, S=sS, C=sC, gamma=p(3), stats=p(4),
               stats_bytes=st_b, dx=p(5), dgamma=p(6), dbeta=p(7), accumulate=0)
    entry("gmz_seg_bn_backward", **sbw, stream=None)
    entry("gmz_seg_bn_backward_small", **sbw, ws=p(8), ws_bytes=sbs_ws, stream=None)
    for fn in ("gmz_seg_bn_forward", "gmz_seg_bn_forward_small", "gmz_seg_bn_backward", "gmz_seg_bn_backward_small"):
        bad(fn, "null", stats=None)
        bad(fn, "nseg", nseg=0)
        bad(fn, "B", B=0)
        bad(fn, "too_large", B=1 << 14, S=1 << 14)  # nseg * B * S * C >= 2^31
        bad(fn, "stats", stats_bytes=st_b - 4)
        bad(fn, "dtype", dtype=7)
    # 33 segments: refused by every entry point but gmz_seg_bn_backward, which has no upper bound and goes on to its
    # statistics check (the buffer sized for 5 segments is then short)
    for fn in ("gmz_seg_bn_forward", "gmz_seg_bn_forward_small", "gmz_seg_bn_backward", "gmz_seg_bn_backward_small"):
        bad(fn, "nseg_33", nseg=33)
    for fn in ("gmz_seg_bn_forward_small", "gmz_seg_bn_backward_small"):
        bad(fn, "C", C=9, stats_bytes=4 * (3 * nseg * 9 + nseg))
        bad(fn, "null_ws", ws=None)
        bad(fn, "workspace", ws_bytes=sbs_ws - 4)
    for fn in ("gmz_seg_bn_forward", "gmz_seg_bn_forward_small"):
        bad(fn, "null_y", y=None)
        bad(fn, "update", update=1, rm=p(9))
    for fn in ("gmz_seg_bn_backward", "gmz_seg_bn_backward_small"):
        bad(fn, "null_dx", dx=None)

    # ------------------------------------------------------------------ gmz_conv.hip
    N = 8  # few boards: the slot and chunk counts below do not depend on the device's CU count
    strides = dict(s0=1152, s1=9, s2=3, s3=1)
    entry("gmz_conv3x3_pack", dtype=1, w=p(1), **strides, transpose=0, packed=p(2), stream=None)
    bad("gmz_conv3x3_pack", "null", packed=None)
    bad("gmz_conv3x3_pack", "dtype", dtype=0)
    bad("gmz_conv3x3_pack", "dtype_7", dtype=7)
    bad("gmz_conv3x3_pack", "unaligned", packed=ODD)
    bad("gmz_conv3x3_pack", "dtype_before_alignment", dtype=7, packed=ODD)
    entry("gmz_conv3x3_pack_job_bytes", out=ctypes.byref(need))
    bad("gmz_conv3x3_pack_job_bytes", "null", out=None)
    entry("gmz_conv3x3_pack_many", dtype=1, jobs=p(1), n_jobs=2, stream=None)
    bad("gmz_conv3x3_pack_many", "null", jobs=None)
    bad("gmz_conv3x3_pack_many", "n_jobs", n_jobs=0)
    bad("gmz_conv3x3_pack_many", "n_jobs_65536", n_jobs=65536)
    bad("gmz_conv3x3_pack_many", "dtype", dtype=0)
    bad("gmz_conv3x3_pack_many", "dtype_7", dtype=7)
    entry("gmz_conv3x3_pack_split", w=p(1), **strides, transpose=0, packed=p(2), stream=None)
    bad("gmz_conv3x3_pack_split", "null", w=None)
    bad("gmz_conv3x3_pack_split", "unaligned", packed=ODD)
    entry("gmz_conv3x3_pack_split_many", jobs=p(1), n_jobs=2, stream=None)
    bad("gmz_conv3x3_pack_split_many", "null", jobs=None)
    bad("gmz_conv3x3_pack_split_many", "n_jobs", n_jobs=65536)
    entry("gmz_conv3x3_forward_split", H=15, x=p(1), packed=p(2), y=p(3), N=N, gamma=p(4), beta=p(5), rm=p(6), rv=p(7),
          eps=1e-4, res=p(8), relu=1, stream=None)
    bad("gmz_conv3x3_forward_split", "null", y=None)
    bad("gmz_conv3x3_forward_split", "N", N=0)
    bad("gmz_conv3x3_forward_split", "plain_with_relu", gamma=None, beta=None, rm=None, rv=None, res=None)
    bad("gmz_conv3x3_forward_split", "bn_without_beta", beta=None)
    bad("gmz_conv3x3_forward_split", "unaligned", res=ODD)
    bad("gmz_conv3x3_forward_split", "alias", y=p(8))
    bad("gmz_conv3x3_forward_split", "size", H=7)
    entry("gmz_conv3x3_stats_slots", N=N, slots=ctypes.byref(chunk))
    bad("gmz_conv3x3_stats_slots", "N", N=0)
    bad("gmz_conv3x3_stats_slots", "null", slots=None)
    slots = _query(lib, "gmz_conv3x3_stats_slots", N, ctype=ctypes.c_int)

    cv = dict(dtype=1, H=15, x=p(1), packed=p(2), y=p(3), N=N, mask=None, stats=p(4), stats_slots=slots)
    entry("gmz_conv3x3_forward_stats", **cv, stream=None)
    entry("gmz_conv3x3_forward_board_stats", **dict(cv, stats_slots=N), stream=None)
    entry("gmz_conv3x3_forward_stamp", **cv, action=p(5), table=p(6), table_dtype=0, table_bytes=4608, stream=None)
    entry("gmz_conv3x3_forward_bnapply", dtype=1, H=15, bn_x=p(1), bn_res=p(2), gamma=p(3), beta=p(4), bn_save=p(5),
          relu=1, bn_y=p(6), packed=p(7), y=p(8), N=N, mask=None, stats=p(9), stats_slots=slots, stream=None)
    entry("gmz_conv3x3_forward", dtype=1, H=15, x=p(1), packed=p(2), y=p(3), N=N, stream=None)
    entry("gmz_conv3x3_forward_add", dtype=1, H=15, x=p(1), packed=p(2), addend=p(3), y=p(4), N=N, stream=None)
    entry("gmz_conv3x3_forward_bwdstats", dtype=1, H=15, x=p(1), packed=p(2), addend=p(3), y=p(4), N=N, mask=None,
          bn_x=p(5), bn_y=p(6), bn_save=p(7), relu=1, stats=p(8), stats_slots=slots, stream=None)
    for fn in ("gmz_conv3x3_forward_stats", "gmz_conv3x3_forward_board_stats", "gmz_conv3x3_forward_stamp",
               "gmz_conv3x3_forward_bnapply", "gmz_conv3x3_forward", "gmz_conv3x3_forward_add",
               "gmz_conv3x3_forward_bwdstats"):
        bad(fn, "null", packed=None)
        bad(fn, "N", N=0)
        bad(fn, "unaligned", y=ODD)
        bad(fn, "dtype", dtype=0)
        bad(fn, "dtype_7", dtype=7)
        bad(fn, "size", H=7)
        bad(fn, "dtype_before_size", dtype=7, H=7)
        if "stats_slots" in base[fn]:
            bad(fn, "slots", stats_slots=base[fn]["stats_slots"] + 1)
            bad(fn, "slots_before_alignment", stats_slots=base[fn]["stats_slots"] - 1, y=ODD)
    bad("gmz_conv3x3_forward_board_stats", "null_stats", stats=None)
    bad("gmz_conv3x3_forward_stamp", "null_action", action=None)
    bad("gmz_conv3x3_forward_stamp", "table_dtype", table_dtype=1, table_bytes=2304)
    bad("gmz_conv3x3_forward_stamp", "table_bytes", table_bytes=2304)
    bad("gmz_conv3x3_forward_stamp", "table_before_slots", table_bytes=2304, stats_slots=slots + 1)
    bad("gmz_conv3x3_forward_stamp", "ab_size_19", H=19)
    bad("gmz_conv3x3_forward_stamp", "ab_size_6", H=6)
    bad("gmz_conv3x3_forward_bnapply", "null_gamma", gamma=None)
    bad("gmz_conv3x3_forward_bnapply", "unaligned_res", bn_res=ODD)
    bad("gmz_conv3x3_forward_bnapply", "alias_in_place", bn_y=p(1))
    bad("gmz_conv3x3_forward_bnapply", "alias_conv_output", y=p(6))
    bad("gmz_conv3x3_forward_add", "null_addend", addend=None)
    bad("gmz_conv3x3_forward_add", "unaligned_addend", addend=ODD)
    bad("gmz_conv3x3_forward_bwdstats", "null_stats", stats=None)
    bad("gmz_conv3x3_forward_bwdstats", "unaligned_addend", addend=ODD)
    bad("gmz_conv3x3_forward_bwdstats", "bn_unaligned", bn_x=ODD)
    bad("gmz_conv3x3_forward_bwdstats", "ab_size_19", H=19)
    bad("gmz_conv3x3_forward_bwdstats", "ab_size_6", H=6)

    entry("gmz_conv3x3_wgrad_workspace_bytes", N=N, out=ctypes.byref(need))
    bad("gmz_conv3x3_wgrad_workspace_bytes", "N", N=0)
    bad("gmz_conv3x3_wgrad_workspace_bytes", "null", out=None)
    wg_ws = _query(lib, "gmz_conv3x3_wgrad_workspace_bytes", N)
    entry("gmz_conv3x3_wgrad", dtype=1, H=15, x=p(1), dy=p(2), N=N, dw=p(3), **strides, accumulate=0, ws=p(4),
          ws_bytes=wg_ws, stream=None)
    bad("gmz_conv3x3_wgrad", "null", dw=None)
    bad("gmz_conv3x3_wgrad", "N", N=0)
    bad("gmz_conv3x3_wgrad", "unaligned", dy=ODD)
    # real host arrays of fake device pointers: the segment tables are read on the host
    segs = (ctypes.c_void_p * 8)
    xs, dys = segs(*[p(10 + i) for i in range(8)]), segs(*[p(20 + i) for i in range(8)])
    dys_null, dys_odd = segs(p(20), None), segs(p(20), ODD)
    build_cases.keep = (xs, dys, dys_null, dys_odd, item_b, chunk, opt_ws, need)  # alive while the cases are called
    entry("gmz_conv3x3_wgrad_segments", dtype=1, H=15, x_segs=xs, dy_segs=dys, nseg=2, n_per_seg=N // 2, dw=p(3),
          **strides, accumulate=0, ws=p(4), ws_bytes=wg_ws, stream=None)
    bad("gmz_conv3x3_wgrad_segments", "null", x_segs=None)
    bad("gmz_conv3x3_wgrad_segments", "nseg", nseg=9)
    bad("gmz_conv3x3_wgrad_segments", "n_per_seg", n_per_seg=0)
    bad("gmz_conv3x3_wgrad_segments", "null_segment", dy_segs=dys_null)
    bad("gmz_conv3x3_wgrad_segments", "unaligned", dy_segs=dys_odd)
    for fn in ("gmz_conv3x3_wgrad", "gmz_conv3x3_wgrad_segments"):
        bad(fn, "size", H=7)
        bad(fn, "workspace", ws_bytes=wg_ws - 4)
        bad(fn, "dtype", dtype=0)
        bad(fn, "dtype_7", dtype=7)
        bad(fn, "size_before_workspace", H=7, ws_bytes=wg_ws - 4)
        bad(fn, "workspace_before_dtype", ws_bytes=wg_ws - 4, dtype=7)
    assert len({c[0] for c in cases}) == len(cases)
    return cases


def run_cases(lib):
    """{case id: [return code, gmz_last_error() text]} of every case of the table."""
    out = {}
    for cid, fn, args in build_cases(lib):
        rc = getattr(lib, fn)(*args)
        out[cid] = [rc, lib.gmz_last_error().decode()]
    return out


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: for machines without a GPU, where no case can launch")
def test_boundary_messages_match_the_recorded_ones():
    import datou_gomoku_muzero_amd._lib as L
    want = json.load(open(FIXTURE))
    for cid, (rc, text) in want.items():
        assert rc == -1 and text and not got_past_validation(text), (cid, rc, text)
    got = run_cases(L.load())
    assert sorted(got) == sorted(want)
    wrong = {cid: (got[cid], want[cid]) for cid in want if got[cid] != want[cid]}
    assert not wrong, wrong


def test_hip_failure_texts_are_recognised():
    """The shape GMZ_HIP gives a failed HIP call's message is told from a validation message."""
    assert got_past_validation("hipGetLastError(): no ROCm-capable device is detected @gmz_train.hip:638")
    assert got_past_validation("hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, st): invalid argument @gmz_conv.hip:7")
    assert got_past_validation("hipGetLastError(): invalid device function @csrc/gmz_heads.hip:207")
    assert not got_past_validation("gmz_bn_forward: workspace of 1656 bytes, needs 1664 (gmz_bn_workspace_bytes)")
    assert not got_past_validation("gmz_conv3x3_forward: dtype must be 1 (f16) or 2 (bf16)")
