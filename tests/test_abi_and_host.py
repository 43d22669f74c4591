"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol the header
declares; the host-side View/MutView/Config logic mirrors engine/src/transformer/mod.rs;
the product never imports the oracle."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent


def header_symbols():
    text = (REPO / "include" / "rama_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rama_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    import rama_amd
    from rama_amd import _lib
    L = rama_amd.load()
    syms = header_symbols()
    assert len(syms) >= 40
    for s in syms:
        assert hasattr(L, s), f"librama_hip.so lacks {s} declared in include/rama_hip.h"
    assert set(syms) == set(_lib.SIGNATURES), set(syms) ^ set(_lib.SIGNATURES)


def test_rust_bindings_declare_every_header_symbol():
    """integration/rust/hip_sys.rs cannot be compiled here (no Rust toolchain); at least it must name every
    entry point of the header exactly once, and nothing the header does not have"""
    text = (REPO / "integration" / "rust" / "hip_sys.rs").read_text()
    declared = re.findall(r"pub fn (rama_[a-z0-9_]+)\s*\(", text)
    assert sorted(declared) == header_symbols(), set(declared) ^ set(header_symbols())
    assert len(declared) == len(set(declared))


def test_tuning_key_table_matches_the_header():
    """every key of rama_set_tuning's table (csrc/rama_api.hip kTuneKeys) is documented in the header's comment on
    rama_set_tuning, and every key quoted there is in the table: 48 keys, none twice"""
    src = (REPO / "rama_amd" / "csrc" / "rama_api.hip").read_text()
    table = re.search(r"kTuneKeys\[\] = \{\n(.*?)\n\};", src, flags=re.S).group(1)
    rows = [r for r in table.split("\n") if r.strip()]
    keys = re.findall(r"^\s*(?:range|one_of|pred)\(\"([a-z0-9_]*)\",", table, flags=re.M)
    assert len(keys) == len(rows), "a row of kTuneKeys the test cannot read"
    assert len(keys) == 48 and len(set(keys)) == 48, sorted(k for k in keys if keys.count(k) > 1)
    header = (REPO / "include" / "rama_hip.h").read_text()
    doc = re.search(r"/\* Modes and performance knobs\..*?\*/\s*int\s+rama_set_tuning\(", header, flags=re.S).group(0)
    assert doc.count("/*") == 1
    documented = set(re.findall(r"\"([a-z0-9_]+)\"", doc))
    assert documented == set(keys), documented ^ set(keys)


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import rama_amd
    with pytest.raises(rama_amd.RamaError):
        rama_amd.Hip(0)


def test_product_does_not_reference_oracle():
    for p in (REPO / "rama_amd").rglob("*"):
        if p.suffix in {".py", ".hip", ".hpp", ".cpp", ".h"}:
            t = p.read_text()
            # comments may NAME the oracle (e.g. "bit-identical to oracle_fill_synth");
            # importing, including, linking or dlopen-ing it is what is forbidden
            bad = re.search(r"^\s*(from|import)\s+\.*oracle|#include\s+[\"<].*oracle|librama_oracle|rama_oracle\.h",
                            t, flags=re.M)
            assert not bad, f"{p} uses the oracle: {bad.group(0)!r}"


def test_range_from_open_end_is_storage_length():
    """mod.rs:44-51: slice(a..) ends at the STORAGE length even on a narrowed view."""
    from rama_amd.transformer import HipSlice, MutView, View
    st = HipSlice(None, 4096, 100, owner=False)
    v = View(st).slice(10, 20)
    assert (v.range.start, v.range.stop) == (10, 20) and len(v) == 10
    w = v.slice(30)                       # absolute offsets, open end = storage length
    assert (w.range.start, w.range.stop) == (30, 100)
    assert w.ptr == 4096 + 4 * 30
    m = MutView(st).mut_slice(5, 7)
    assert m.as_view().ptr == 4096 + 20 and len(m) == 2


def test_config_from_file_sign_of_vocab(tmp_path, golden_dir):
    import rama_amd
    c = rama_amd.Config.from_file(golden_dir / "ckpt_tied.bin")
    assert c.shared_weight and c.vocab_size == 64 and c.dim == 32 and c.seq_len == 16
    c = rama_amd.Config.from_file(golden_dir / "ckpt_untied.bin")
    assert (not c.shared_weight) and c.vocab_size == 64
    short = tmp_path / "short.bin"
    short.write_bytes(b"\x00" * 12)
    with pytest.raises(rama_amd.RamaError):
        rama_amd.Config.from_file(short)


def test_algorithmic_bytes_match_baseline_table():
    import rama_amd
    # BASELINE.md section 2
    for dims, want in [((288, 768, 6, 6, 32000, 256), 60_751_872),
                       ((768, 2048, 12, 12, 32000, 1024), 438_042_624),
                       ((4096, 11008, 32, 32, 32000, 2048), 26_428_309_504)]:
        d, h, L, H, V, S = dims
        cfg = rama_amd.Config(d, h, L, H, H, V, S, True)
        assert rama_amd.algorithmic_bytes(cfg)["token"] == want
