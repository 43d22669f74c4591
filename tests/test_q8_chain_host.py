"""CPU-side checks (no GPU) of the chained Q8 batch: the four entry points are declared, bound and exported, rama_q8_seq_plan
has the C layout, and rama_amd.q8.decode_batch_chained refuses bad arguments before any library call."""
import ctypes as C
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import pytest

REPO = Path(__file__).resolve().parent.parent
ENTRIES = ("rama_q8_decode_batch_begin", "rama_q8_decode_batch_steps", "rama_q8_decode_batch_tokens", "rama_q8_decode_batch_stream_poll")


def header_text():
    return re.sub(r"/\*.*?\*/", "", (REPO / "include" / "rama_hip.h").read_text(), flags=re.S)


def test_entries_declared_bound_and_exported():
    import rama_amd
    from rama_amd import _lib
    declared = set(re.findall(r"\b(rama_[a-z0-9_]+)\s*\(", header_text()))
    L = rama_amd.load()
    for s in ENTRIES:
        assert s in declared, f"include/rama_hip.h does not declare {s}"
        assert s in _lib.SIGNATURES, f"rama_amd/_lib.py does not bind {s}"
        assert hasattr(L, s), f"librama_hip.so lacks {s}"
    rust = (REPO / "integration" / "rust" / "hip_sys.rs").read_text()
    for s in ENTRIES:
        assert len(re.findall(rf"pub fn {s}\s*\(", rust)) == 1, s


def test_signatures_match_the_header():
    """argument counts of the four prototypes, and the plan pointer / the finished pointer where the header has them"""
    from rama_amd import _lib
    text = header_text()
    for s in ENTRIES:
        args = re.search(rf"\b{s}\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        res, argtypes = _lib.SIGNATURES[s]
        assert res is C.c_int and len(argtypes) == args.count(",") + 1, s
    assert _lib.SIGNATURES["rama_q8_decode_batch_begin"][1][-1] is C.POINTER(_lib.rama_q8_seq_plan)
    assert _lib.SIGNATURES["rama_q8_decode_batch_stream_poll"][1][-2:] == [C.POINTER(C.c_int), C.POINTER(C.c_int)]


def test_seq_plan_layout_matches_c(tmp_path):
    """sizeof and every offsetof of rama_q8_seq_plan as the C compiler lays the header's struct out"""
    from rama_amd._lib import rama_q8_seq_plan
    fields = [f[0] for f in rama_q8_seq_plan._fields_]
    assert fields == ["temperature", "topp", "u", "forced", "n_forced", "max_new", "stop_token"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rama_hip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(rama_q8_seq_plan));\n' +
                   "".join(f'    printf(" %zu", offsetof(rama_q8_seq_plan, {f}));\n' for f in fields) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", str(REPO / "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(rama_q8_seq_plan)
    assert got[1:] == [getattr(rama_q8_seq_plan, f).offset for f in fields]
    for f, t in (("temperature", C.c_float), ("n_forced", C.c_int32), ("max_new", C.c_int32), ("stop_token", C.c_int32)):
        assert getattr(rama_q8_seq_plan, f).size == C.sizeof(t)
    assert rama_q8_seq_plan.forced.size == C.sizeof(C.c_void_p)


class NoDevice:
    """stands where an engine's Hip would: any use of the library is a failure of the test"""

    def __getattr__(self, name):
        raise AssertionError(f"decode_batch_chained touched the device ({name}) before refusing its arguments")


def fake_engines(n, model=None, vocab_size=64, seq_len=32):
    model = model or SimpleNamespace(name="m")
    cfg = SimpleNamespace(vocab_size=vocab_size, seq_len=seq_len)
    return [SimpleNamespace(model=model, cfg=cfg, device=NoDevice(), state=None) for _ in range(n)]


def test_chained_wrapper_refuses_bad_arguments_without_a_device():
    from rama_amd.q8 import chain_plan, decode_batch_chained as run
    e = fake_engines(3)
    V, S = 64, 32
    bad = [
        dict(tokens=[1, 2], positions=[0, 0, 0]),                                        # mismatched lengths
        dict(tokens=[1, 2, 3], positions=[0, 0]),
        dict(temperature=[0.0, 1.0]),
        dict(topp=[0.9] * 4),
        dict(u=[0.1]),
        dict(prompts=[[1], [2]]),
        dict(max_new=[1, 2]),
        dict(stop_tokens=[1, 2, 3, 4]),
        dict(tokens=[1, V, 3]),                                                          # outside the vocabulary
        dict(tokens=[-1, 2, 3]),
        dict(prompts=[[1, 2], [3, V], []]),
        dict(prompts=[[-2], [], []]),
        dict(stop_tokens=[None, V, None]),
        dict(stop_tokens=-2),
        dict(positions=[0, S - 3, 0]),                                                   # position + budget past seq_len (4 steps)
        dict(positions=[0, -1, 0]),
        dict(positions=[0, S - 2, 0], max_new=[None, 3, None]),
        dict(positions=[0, S, 0], max_new=1),
        dict(max_new=[0, -1, 0]),
        dict(temperature=-0.5),
        dict(temperature=float("nan")),
        dict(topp=1.5),
        dict(u=1.0),
        dict(n_steps=0),
    ]
    for kw in bad:
        args = dict(tokens=[1, 2, 3], positions=[0, 1, 2], n_steps=4)
        args.update(kw)
        with pytest.raises(ValueError):
            run(e, **args)
    with pytest.raises(ValueError):                                                      # more than 128 sequences
        run(fake_engines(129), [1] * 129, [0] * 129, 2)
    with pytest.raises(ValueError):
        run([], [], [], 2)
    with pytest.raises(ValueError):                                                      # engines of different models
        run([e[0], fake_engines(1)[0]], [1, 2], [0, 0], 2)
    with pytest.raises(ValueError):                                                      # the same engine twice
        run([e[0], e[1], e[0]], [1, 2, 3], [0, 0, 0], 2)
    # what is accepted: a budget that ends exactly at seq_len, per-sequence values, None entries
    toks, poss, plan = chain_plan(e, [1, 2, 3], [S - 4, S - 2, S - 1], 4, temperature=[0.0, 1.0, 0.7], topp=[0.9, 0.9, 0.5],
                                  u=[0.0, 0.25, 0.5], prompts=[[1, 5], None, []], max_new=[None, 2, 1], stop_tokens=[None, 7, V - 1])
    assert (toks, poss) == ([1, 2, 3], [S - 4, S - 2, S - 1])
    assert plan == [(0.0, 0.9, 0.0, [1, 5], 0, -1), (1.0, 0.9, 0.25, [], 2, 7), (0.7, 0.5, 0.5, [], 1, V - 1)]
