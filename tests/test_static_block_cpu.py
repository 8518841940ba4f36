"""Layout of the captured step's static block (``train_model._StaticBlock``) on the CPU: the
device tensor and its host image carry the same four named views at the same word offsets."""
import os
import re

import numpy as np
import pytest
import torch

import pcgmix_amd  # noqa: F401
from pcgmix_amd import train_model as tm


def _granules(B):
    return 16 * ((B + 15) // 16)


def _byte_offset(view, base):
    if isinstance(view, torch.Tensor):
        return view.data_ptr() - base.data_ptr()
    return view.ctypes.data - base.ctypes.data


@pytest.mark.parametrize("B,classes", [(1, 2), (15, 2), (16, 2), (17, 2), (256, 2), (16, 3)])
def test_static_block_layout(B, classes):
    blk = tm._StaticBlock(B, classes, "cpu")
    dev = (blk.key, blk.hyper, blk.labels, blk.targets)
    host = (blk.host_key, blk.host_hyper, blk.host_labels, blk.host_targets)
    lab_bytes = _granules(B)
    t_at = 48 + lab_bytes
    # the same offsets in both copies: key at word 0, Adam scalars at word 4, label bytes at byte 48
    # (16-byte granules), float targets behind them on a 4-word boundary
    assert [_byte_offset(v, blk.dev) for v in dev] == [0, 16, 48, t_at]
    assert [_byte_offset(v, blk.host) for v in host] == [0, 16, 48, t_at]
    assert t_at % 16 == 0
    for key, hyper, labels, targets in (dev, host):
        assert tuple(key.shape) == (2,) and key.dtype in (torch.int32, np.uint32)
        assert tuple(hyper.shape) == (8,) and hyper.dtype in (torch.float32, np.float32)
        assert tuple(labels.shape) == (B,) and labels.dtype in (torch.uint8, np.uint8)
        assert tuple(targets.shape) == (B, classes) and targets.dtype in (torch.float32, np.float32)
    assert blk.dev.dtype == torch.float32 and blk.host.dtype == np.float32
    assert blk.dev.numel() == blk.host.size
    # the payload: up to the end of the label granules for hard labels, else the whole block, whose
    # targets are padded to 4 words
    assert blk.payload_bytes(True) == 48 + lab_bytes
    assert blk.payload_bytes(False) == blk.host.nbytes == blk.dev.numel() * 4
    assert blk.host.nbytes == t_at + 16 * ((B * classes + 3) // 4)
    # placeholder targets on the device: one-hot rows of class 0
    assert torch.equal(blk.targets[:, 0], torch.ones(B)) and float(blk.targets.sum()) == B
    assert not blk.host.any()


def test_static_block_hard_label_payload_fits_the_kernel_arguments():
    """B = 256: 304 bytes, within ``kPackPayBytes`` of csrc/pcgmix_kernels.h."""
    header = os.path.join(os.path.dirname(tm.__file__), "csrc", "pcgmix_kernels.h")
    limit = int(re.search(r"kPackPayBytes\s*=\s*(\d+)", open(header).read()).group(1))
    assert limit == 320
    assert tm._StaticBlock(256, 2, "cpu").payload_bytes(True) == 304 <= limit


@pytest.mark.parametrize("B,classes", [(1, 2), (17, 2), (16, 3)])
def test_static_block_views_do_not_overlap(B, classes):
    """Writing through one named view changes that view's bytes and no others, in either copy."""
    blk = tm._StaticBlock(B, classes, "cpu")
    blk.targets.zero_()
    f = float(np.frombuffer(b"\x11\x22\x33\x44", np.float32)[0])       # no zero byte: every byte changes
    fills = (lambda v: v.fill_(-1) if isinstance(v, torch.Tensor) else v.fill(0xFFFFFFFF),   # key
             lambda v: v.fill_(f) if isinstance(v, torch.Tensor) else v.fill(f),             # hyper
             lambda v: v.fill_(255) if isinstance(v, torch.Tensor) else v.fill(255),         # labels
             lambda v: v.fill_(f) if isinstance(v, torch.Tensor) else v.fill(f))             # targets
    spans = ((0, 8), (16, 48), (48, 48 + B), (48 + _granules(B), 48 + _granules(B) + 4 * B * classes))
    for views, words in (((blk.key, blk.hyper, blk.labels, blk.targets), blk.dev.numpy()),
                         ((blk.host_key, blk.host_hyper, blk.host_labels, blk.host_targets), blk.host)):
        raw = words.view(np.uint8)
        for view, fill, (lo, hi) in zip(views, fills, spans):
            before = raw.copy()
            fill(view)
            changed = np.flatnonzero(raw != before)
            assert changed.size == hi - lo and changed[0] == lo and changed[-1] == hi - 1
