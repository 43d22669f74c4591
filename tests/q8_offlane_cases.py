"""The Q8 models that leave the fast kernels (tests/test_hip_q8_offlane.py, tests/test_q8_host.py): shapes as data.

Paths are the values of rama_q8_product_path (include/rama_hip.h)."""
MATVEC, MATVEC_GENERIC, GEMM_KSPLIT, GEMM_MFMA, GEMM_GENERIC = 0, 1, 2, 3, 4

# the two exporter-written fixtures (tools/make_q8_goldens.py): the exporter halves the group size until it divides dim
FIXTURE_CFGS = {
    "ckpt_v2_q80_gs16": (dict(dim=48, hidden_dim=80, n_layers=2, n_heads=3, n_kv_heads=3, vocab_size=50, seq_len=40, shared_weight=True), 16),
    "ckpt_v2_q80_gs8": (dict(dim=72, hidden_dim=200, n_layers=2, n_heads=2, n_kv_heads=2, vocab_size=37, seq_len=24, shared_weight=False), 8),
}
# a synthetic model at group size 128: two chunks of 64 bytes per group on the matrix-core kernel
GS128_CFG = dict(dim=256, hidden_dim=640, n_layers=2, n_heads=4, n_kv_heads=4, vocab_size=131, seq_len=48, shared_weight=True)
GS128_SEED = 21
# one layer whose context is too long for the chain attention's score buffer: seq_len is the smallest multiple of 1024 for
# which rama_q8_batch_shape_ok is false (found by calling it; the tests assert it).  The score and probability rows of
# attention_chain_kernel take 2 x seq_len floats of its 136 KiB.
LONGCTX_SEQ_LEN = 8192
LONGCTX_CFG = dict(dim=64, hidden_dim=192, n_layers=1, n_heads=2, n_kv_heads=2, vocab_size=64, seq_len=LONGCTX_SEQ_LEN, shared_weight=True)
LONGCTX_GS, LONGCTX_SEED = 32, 9
# the same shape at the longest context launch_attention_ref takes (its score row is 64 KiB of LDS: a longer one is
# RAMA_EUNSUP from every Q8 entry, so no position past 16384 exists), and its last position
LONGCTX_DEEP_SEQ_LEN = 16384
LONGCTX_DEEP_POS = 16383
LONGCTX_REFUSED_SEQ_LEN = 17408

# model -> the group size, every K its products have, the matvec path of each K and the batch path at every token count
MODEL_PATHS = {
    "ckpt_v2_q80_gs16": dict(gs=16, matvec={48: MATVEC, 80: MATVEC}, gemm=GEMM_GENERIC),
    "ckpt_v2_q80_gs8": dict(gs=8, matvec={72: MATVEC_GENERIC, 200: MATVEC_GENERIC}, gemm=GEMM_GENERIC),
    "gs128": dict(gs=128, matvec={256: MATVEC, 640: MATVEC}, gemm=GEMM_MFMA),
}
TOKEN_COUNTS = (1, 2, 5, 16, 17, 32, 33, 64, 65, 128, 130)

STORIES15M = dict(dim=288, hidden_dim=768, n_layers=6, n_heads=6, n_kv_heads=6, vocab_size=32000, seq_len=256, shared_weight=True)
