"""The wide workloads of the serving chain (data only; no test, no GPU): the slot and row counts above what
tests/test_hip_q8_serve.py starts -- the scheduler's second wave, the classifier's ksplit<2> and one-wave MFMA forms over the
gathered rows, the layer pass at 17..64 rows.  tests/test_q8_serve_wide_host.py replays every workload with the host plan and
asserts that it reaches what it is for; tests/test_hip_q8_serve_wide.py runs it on the GPU.

A workload: the model, n_slots, max_rows, the graph modes, the slots left FREE, and per occupied slot -- ascending slot index --
(context length, max_new, plan kind).  The sizes come from one numpy generator per workload (its seed is in the table): a
context is 1 token with probability p_one (such a slot decodes from its second step on, and takes none of the rows left
over), else uniform in 2..ctx_max; max_new is uniform in 1..new_max, cut to what seq_len leaves.  The plan kinds are
those tests.test_hip_q8_serve.mixed_requests gives the k-th request of a list: the sampler records in turn, and every third
request -- where its budget is 3 or more -- stops on a token of its own solo run."""
from collections import namedtuple

import numpy as np

SEQ_LEN = dict(ckpt_v2_q80_tied=16, ckpt_v2_q80_untied=32, synth15m=256)
SAMPLERS = [(0.0, 0.9, 0.0), (1.0, 0.9, 0.1), (0.7, 0.5, 0.6), (0.0, 0.9, 0.0), (1.0, 0.95, 0.83)]      # mixed_requests' own

Wide = namedtuple("Wide", "model n_slots max_rows graphs holes seed p_one ctx_max new_max sizes")


def plan_kind(k, max_new):
    """the k-th request of mixed_requests: 'greedy' / 'sampled', + '+stop' where it stops on a token of its solo run"""
    kind = "sampled" if SAMPLERS[k % len(SAMPLERS)][0] > 0.0 else "greedy"
    return kind + ("+stop" if k % 3 == 1 and max_new >= 3 else "")


def _wide(model, n_slots, max_rows, graphs, holes, seed, p_one, ctx_max, new_max):
    rng = np.random.default_rng(seed)
    sizes = []
    for k in range(n_slots - len(holes)):
        n_ctx = 1 if rng.random() < p_one else int(rng.integers(2, ctx_max + 1))
        new = min(int(rng.integers(1, new_max + 1)), SEQ_LEN[model] - n_ctx)
        sizes.append((n_ctx, new, plan_kind(k, new)))
    return Wide(model, n_slots, max_rows, tuple(graphs), tuple(sorted(holes)), seed, p_one, ctx_max, new_max, tuple(sizes))


#                 model           n_slots max_rows graphs  FREE holes          seed  p_one ctx_max new_max
WORKLOADS = [
    _wide("ckpt_v2_q80_tied",        17,   17, (0, 1), (),                 1701, 0.3, 12, 8),
    _wide("ckpt_v2_q80_tied",        33,   33, (0, 1), (7,),               3301, 0.3, 12, 8),
    _wide("ckpt_v2_q80_tied",        64,   64, (0, 1), (0, 63),            6401, 0.3, 12, 8),
    _wide("ckpt_v2_q80_tied",        65,   70, (0, 1), (5, 62),            6515, 0.7, 13, 8),
    _wide("ckpt_v2_q80_tied",       128,  128, (0, 1), (0, 63, 64, 127),  12801, 0.7, 13, 8),
    _wide("ckpt_v2_q80_tied",        40,   64, (0, 1), (3, 39),            4001, 0.3, 12, 8),
    _wide("ckpt_v2_q80_untied",      24,   32, (0, 1), (11,),              2401, 0.3, 20, 10),
    _wide("ckpt_v2_q80_untied",      65,   96, (0, 1), (0, 31),            6502, 0.5, 24, 8),
    _wide("ckpt_v2_q80_untied",     128,  128, (0, 1), (0, 63, 64, 127),  12802, 0.7, 24, 8),
    _wide("synth15m",                33,   48, (1,),   (16,),              3302, 0.3, 40, 8),
    _wide("synth15m",                65,   96, (0,),   (0, 40),            6512, 0.5, 40, 8),
    _wide("synth15m",               128,  128, (1,),   (0, 63, 64, 127),  12803, 0.7, 32, 6),
]


def case_id(w):
    return f"{w.model}-{w.n_slots}x{w.max_rows}"


def occupied(w):
    """the occupied slot indices, ascending: sizes[k] belongs to occupied(w)[k]"""
    return [i for i in range(w.n_slots) if i not in w.holes]
