#!/usr/bin/env python3
"""Generate the Q8_0 (llama2.c version-2) fixtures of tests/golden/ with the REFERENCE's own exporter.

Runs only in the build container, like tools/make_goldens.py: it imports the reference's model.py and
export.py at run time and writes data only -- four tiny torch-initialised models written by
``export.version2_export`` and, next to each, an ``.npz`` with some of the fp32 weights it quantized (v0
tensor names and shapes: the token table, wq, w2, the norms, an untied classifier), the config, the group size and the exporter's max error.

* ckpt_v2_q80_tied.bin    the make_ckpt_case shape (dim 32, hidden 96): the group size backs off 64 -> 32
* ckpt_v2_q80_untied.bin  dim 64, hidden 192, 4 heads, seq_len 32, group size 64, non-unit norm gains
* ckpt_v2_q80_gs16.bin    dim 48, hidden 80, 3 heads, vocab 50, seq_len 40, tied: the group size backs off 64 -> 32 -> 16
* ckpt_v2_q80_gs8.bin     dim 72, hidden 200, 2 heads (head size 36), vocab 37, seq_len 24, untied: the group size backs off
                          to 8, and no row is a multiple of 16 bytes (the bytewise kernels' model)

Usage:  python tools/make_q8_goldens.py
"""
from __future__ import annotations

import contextlib
import io
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
REF_EXPORT = Path("/root/reference/engine/export")
sys.path.insert(0, str(REF_EXPORT))

import model as ref_model      # noqa: E402  (reference, container-only)
import export as ref_export    # noqa: E402

OUT = REPO / "tests" / "golden"
# the fp32 tensors the .npz keeps (the tests compare these with the file): the token table, one attention and one FFN matrix,
# the norms, and the classifier of the untied model
KEEP = ("token_embedding_table", "wq", "w2", "rms_att_weight", "rms_ffn_weight", "rms_final_weight")


def build(dim, hidden, n_layers, n_heads, vocab, seq_len, shared, seed):
    torch.manual_seed(seed)
    args = ref_model.ModelArgs(dim=dim, n_layers=n_layers, n_heads=n_heads, n_kv_heads=None, vocab_size=vocab,
                               hidden_dim=hidden, multiple_of=32, max_seq_len=seq_len, dropout=0.0)
    m = ref_model.Transformer(args)
    m.eval()
    with torch.no_grad():
        if not shared:
            m.output.weight = torch.nn.Parameter(torch.randn(vocab, dim) * 0.02)
            m.tok_embeddings.weight = torch.nn.Parameter(m.tok_embeddings.weight.detach().clone())
        for layer in m.layers:       # non-unit norm gains so a norm mix-up cannot hide
            layer.attention_norm.weight.add_(torch.randn(dim) * 0.1)
            layer.ffn_norm.weight.add_(torch.randn(dim) * 0.1)
        m.norm.weight.add_(torch.randn(dim) * 0.1)
    return m


def fp32_weights(m) -> dict:
    f = lambda t: t.detach().float().numpy().astype(np.float32)
    st = lambda get: np.stack([f(get(l)) for l in m.layers])
    w = dict(token_embedding_table=f(m.tok_embeddings.weight),
             rms_att_weight=st(lambda l: l.attention_norm.weight), rms_ffn_weight=st(lambda l: l.ffn_norm.weight),
             wq=st(lambda l: l.attention.wq.weight), wk=st(lambda l: l.attention.wk.weight),
             wv=st(lambda l: l.attention.wv.weight), wo=st(lambda l: l.attention.wo.weight),
             w1=st(lambda l: l.feed_forward.w1.weight), w2=st(lambda l: l.feed_forward.w2.weight),
             w3=st(lambda l: l.feed_forward.w3.weight), rms_final_weight=f(m.norm.weight), wcls=f(m.output.weight))
    return w


def make(name, shared, seed, want_gs, **shape):
    m = build(shared=shared, seed=seed, **shape)
    w = fp32_weights(m)
    path = OUT / f"{name}.bin"
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        ref_export.version2_export(m, str(path), group_size=64)
    maxerr = max(float(ln.rsplit(" ", 1)[1]) for ln in log.getvalue().splitlines() if "with max error" in ln)
    gs = int(np.frombuffer(path.read_bytes()[37:41], "<i4")[0])
    if gs != want_gs:
        sys.exit(f"{name}: the exporter wrote group size {gs}, the fixture is meant to have {want_gs}")
    cfg = np.array([shape["dim"], shape["hidden"], shape["n_layers"], shape["n_heads"], shape["n_heads"], shape["vocab"],
                    shape["seq_len"], int(shared)], np.int32)
    keep = {k: w[k] for k in KEEP + (("wcls",) if not shared else ())}
    np.savez_compressed(OUT / f"{name}.npz", cfg=cfg, group_size=np.int32(gs), maxerr=np.float32(maxerr), **keep)
    print(name, "bytes", path.stat().st_size, "group_size", gs, "maxerr", maxerr)


if __name__ == "__main__":
    make("ckpt_v2_q80_tied", True, 1234, 32, dim=32, hidden=96, n_layers=2, n_heads=2, vocab=64, seq_len=16)
    make("ckpt_v2_q80_untied", False, 4321, 64, dim=64, hidden=192, n_layers=2, n_heads=4, vocab=64, seq_len=32)
    make("ckpt_v2_q80_gs16", True, 1616, 16, dim=48, hidden=80, n_layers=2, n_heads=3, vocab=50, seq_len=40)
    make("ckpt_v2_q80_gs8", False, 808, 8, dim=72, hidden=200, n_layers=2, n_heads=2, vocab=37, seq_len=24)
