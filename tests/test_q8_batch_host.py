"""Q8 token batches without a GPU: the Python wrappers refuse bad arguments before any library call, and the three
new entries are declared in the header, the ctypes table and the Rust bindings."""
import re
from pathlib import Path

import pytest

from rama_amd import _lib
from rama_amd.q8 import Q8Engine, decode_batch
from rama_amd.transformer import Config

REPO = Path(__file__).resolve().parent.parent
NEW = ("rama_q8_matmul_batch", "rama_q8_prefill", "rama_q8_decode_batch")


class NoDevice:
    """a device whose library must never be reached"""

    ctx = None

    @property
    def lib(self):
        raise AssertionError("the wrapper reached the library before refusing its arguments")


class FakeModel:
    def __init__(self):
        self.cfg = Config(64, 192, 2, 4, 4, 64, 32, False)


def fake_engine(model):
    e = object.__new__(Q8Engine)
    e.device, e.model, e.cfg = NoDevice(), model, model.cfg
    e.state = _lib.rama_run_state()
    return e


def test_prefill_refuses_before_the_device():
    e = fake_engine(FakeModel())
    for toks, pos0 in (([], 0), ([1, 2], -1), ([1] * 33, 0), ([1, 2], 31), ([1, 64], 0), ([-1], 0)):
        with pytest.raises(ValueError):
            e.prefill(toks, pos0)


def test_decode_batch_refuses_before_the_device():
    m = FakeModel()
    a, b = fake_engine(m), fake_engine(m)
    cases = [
        ([], [], []),                                     # no sequences
        ([a, b], [1], [0, 0]),                            # lengths differ
        ([a, b], [1, 1], [0]),
        ([a, a], [1, 1], [0, 1]),                         # one state twice
        ([a, fake_engine(FakeModel())], [1, 1], [0, 0]),  # two models
        ([a, b], [1, 64], [0, 0]),                        # token outside the vocabulary
        ([a, b], [-1, 1], [0, 0]),
        ([a, b], [1, 1], [0, 32]),                        # position outside [0, seq_len)
        ([a, b], [1, 1], [-1, 0]),
        ([fake_engine(m) for _ in range(129)], [1] * 129, [0] * 129),
    ]
    for engs, toks, poss in cases:
        with pytest.raises(ValueError):
            decode_batch(engs, toks, poss)


def test_new_entries_declared_everywhere():
    header = (REPO / "include" / "rama_hip.h").read_text()
    rust = (REPO / "integration" / "rust" / "hip_sys.rs").read_text()
    for name in NEW:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
        assert re.search(rf"pub fn {name}\(", rust), name
    # argument counts agree between the header and the ctypes table
    for name in NEW:
        decl = re.search(rf"\b{name}\(([^;]*)\);", header, re.S).group(1)
        assert decl.count(",") + 1 == len(_lib.SIGNATURES[name][1]), name
