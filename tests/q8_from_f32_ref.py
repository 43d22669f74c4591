"""What rama_q8_model_from_f32 must give, restated in numpy: export.py's quantize_q80 rule over an fp32 weight dict (the oracle's names),
every layer's matrix on its own, and version2_export's group-size back-off.  No GPU, nothing of rama_amd imported."""
import numpy as np

# Q8 tensor name -> (fp32 weight name, stacked over the layers)
SOURCES = dict(tok=("token_embedding_table", False), wq=("wq", True), wk=("wk", True), wv=("wv", True), wo=("wo", True), w1=("w1", True),
               w2=("w2", True), w3=("w3", True), wcls=("wcls", False))
NORMS = ("rms_att_weight", "rms_ffn_weight", "rms_final_weight")


def group_size(dim: int, hidden_dim: int, wanted: int = 64) -> int:
    """halve the wanted size while it does not divide dim (version2_export) or hidden_dim (every row of W2 is whole groups)"""
    gs = int(wanted)
    while gs > 1 and (dim % gs or hidden_dim % gs):
        gs //= 2
    return gs


def quantize_groups(w, gs: int):
    """-> (int8 values, fp32 scales) of a flat fp32 array: per group of gs values scale = max|w| / 127 in fp32, q = round-half-even(w / scale)
    in fp32, clamped to [-127, 127]; a zero scale gives zeros"""
    a = np.ascontiguousarray(w, np.float32).reshape(-1, gs)
    scale = (np.abs(a).max(axis=1) / np.float32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.rint((a / scale[:, None]).astype(np.float32))
    r = np.where(scale[:, None] == 0, np.float32(0), r)
    q = np.clip(r, -127, 127).astype(np.int8)
    return q.reshape(-1), scale


def from_f32(cfg, w: dict, gs: int):
    """-> (tensors: name -> (int8 values, scales), norms: name -> fp32, the dequantized fp32 token table); wcls is tok's pair when shared"""
    L = cfg.n_layers
    t = {}
    for name, (src, layered) in SOURCES.items():
        if name == "wcls" and cfg.shared_weight:
            t[name] = t["tok"]
            continue
        a = np.ascontiguousarray(w[src], np.float32).reshape(-1)
        if layered:                                               # every layer's matrix on its own, then stacked
            parts = [quantize_groups(p, gs) for p in a.reshape(L, -1)]
            t[name] = (np.concatenate([q for q, _ in parts]), np.concatenate([s for _, s in parts]))
        else:
            t[name] = quantize_groups(a, gs)
    norms = {n: np.ascontiguousarray(w[n], np.float32).reshape(-1) for n in NORMS}
    q, s = t["tok"]
    table = (q.astype(np.float32).reshape(-1, gs) * s[:, None]).astype(np.float32).reshape(-1)
    return t, norms, table
