"""rama_set_tuning: which values every key accepts and refuses, and that nothing but the 48 keys is a key.

The table below is written out by hand from the C ABI's documented and implemented domains; it is not derived from the
library's own key table, so a row dropped or a bound moved there shows up here."""
import pytest

import rama_amd
from rama_amd import _lib

pytestmark = pytest.mark.gpu

RAMA_EINVAL = -1
INT_MAX, INT_MIN = 2**31 - 1, -2**31

SWITCH = ((0, 1), (-1, 2))               # 0|1
TRISTATE = ((-1, 0, 1), (-2, 2))         # -1|0|1

# key: (accepted values -- both ends of the domain and the default --, the nearest refused values on each side)
KEYS = {
    "ref_order": ((0, 1, 2, 3), (-1, 4)),
    "lane_reduce": ((0, 1, 2), (-1, 3)),
    "bar_pos": ((0, 128, INT_MAX), (-1, INT_MIN)),
    "tol_mask": ((0, 127), (-1, 128)),
    "geom": ((0, 3, 4), (-1, 5)),
    "resid_r2": ((0, 2, 3), (-1, 4)),
    "solo": TRISTATE,
    "w13i": SWITCH,
    "fused": TRISTATE,
    "fused_solo": TRISTATE,
    "merge": TRISTATE,
    "split_pos": ((-1, 0, 256, INT_MAX), (-2, INT_MIN)),
    "attn_nsplit": ((0, 1, 32), (-1, 33)),
    "attn_waves": ((4, 8, 16), (3, 5, 7, 9, 15, 17, 0)),
    "attn_nt": SWITCH,
    "attn_u": ((8, 16), (7, 9, 15, 17, 0)),
    "combine_v": SWITCH,
    "small_attn": TRISTATE,
    "small_attn_waves": ((4, 8), (3, 5, 7, 9, 0)),
    "small_attn_pos": ((0, 256, INT_MAX), (-1, INT_MIN)),
    "graph_steps": ((-1, 1, 32), (-2, 0, 33)),
    "prefill": SWITCH,
    "prefill_tok": ((64, 128), (0, 63, 65, 96, 127, 129, 256)),
    "prefill_attn": SWITCH,
    "tiled": SWITCH,
    "norm_in_gemm": SWITCH,
    "topp_sort": SWITCH,
    "topp_pairs": SWITCH,
    "topp_dist": SWITCH,
    "topp_block": ((512, 1024, 2048), (0, 511, 513, 1023, 1025, 2047, 2049)),
    "topp_keep_sums": ((1, 0), (-1, 2)),
    "chain": SWITCH,
    "chain_d": ((0, 116, 216, 432), (-1, 1, 115, 433)),
    "chain_resid_d": ((-1, 0, 116, 132, 216, 232, 416, 432), (-2, 1, 100, 115, 117, 124, 316, 332, 516, 532)),
    "chain_lead_w": ((0, 1, 2), (-1, 3)),
    "chain_norm": SWITCH,
    "chain_lead": SWITCH,
    "chain_split": SWITCH,
    "chain_views": SWITCH,
    "spread_pos": ((64, 128, 1 << 20), (63, (1 << 20) + 1, 0, -1)),
    "attn_fv": SWITCH,
    "prefill_chain": SWITCH,
    "rope_batch": SWITCH,
    "matmul_batch": SWITCH,
    "ew_batch": SWITCH,
    "norm_fold": SWITCH,
    "resid_fold": SWITCH,
    "qkv_fold": SWITCH,
}

NOT_KEYS = ("", "nope", "fuse", "fused_", "chain_dd", "Geom", "geom ", " geom", "tune_geom")


@pytest.fixture(scope="module")
def dev():
    d = rama_amd.Hip(0)      # a context of its own: nothing set here reaches another test
    yield d
    d.close()


def set_tuning(dev, key, value):
    rc = dev.lib.rama_set_tuning(dev.ctx, None if key is None else key.encode(), value)
    return rc, (dev.lib.rama_last_error() or b"").decode()


def test_table_has_the_48_keys():
    assert len(KEYS) == 48


@pytest.mark.parametrize("key", sorted(KEYS))
def test_key_domain(dev, key):
    accepted, refused = KEYS[key]
    for v in refused:
        rc, msg = set_tuning(dev, key, v)
        print(f"{key} = {v}: rc {rc} {msg!r}")
        assert rc == RAMA_EINVAL, f"{key} = {v} was not refused (rc {rc})"
        assert msg, f"{key} = {v} refused without a message"
    for v in accepted + accepted[::-1]:      # every accepted value, also after another one
        rc, msg = set_tuning(dev, key, v)
        assert rc == 0, f"{key} = {v} refused (rc {rc}): {msg}"
    rc, _ = set_tuning(dev, key, refused[0])      # ... and a refusal after values were accepted
    assert rc == RAMA_EINVAL
    dev.sync()


@pytest.mark.parametrize("key", NOT_KEYS)
def test_unknown_key_is_refused(dev, key):
    for v in (0, 1):
        rc, msg = set_tuning(dev, key, v)
        assert rc == RAMA_EINVAL, f"{key!r} was taken for a key (rc {rc})"
        assert msg


def test_null_arguments_are_refused(dev):
    rc, msg = set_tuning(dev, None, 0)
    assert rc == RAMA_EINVAL and msg
    assert _lib.load().rama_set_tuning(None, b"geom", 3) == RAMA_EINVAL
