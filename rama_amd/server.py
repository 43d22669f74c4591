"""rama_amd.Server -- continuous batching over an fp32 Model in parity mode (rama_serve_*): the counterpart of
Q8Server.  Both are rama_amd.serve.ServeLoop -- the queue, the mirror of the slot table, the steps to the next finish by the host plan,
admissions behind the steps in flight, the rings, the prefix cache and the run loop of a chain with drafts -- over their own entries and
engines."""
from __future__ import annotations

from .engine import Engine, Model
from .q8 import Q8Engine, Q8Model
from .serve import ServeLoop


class Server(ServeLoop):
    """n_slots sequence slots share parity-mode weight passes of max_rows rows (tiles of 32).  Every request's tokens are those
    Engine.generate gives it alone in parity mode -- the reference's own.  The device context must be in parity mode
    ("ref_order" = 1) and stay there.  One fp32 serving chain per device context; a Q8Server may be live next to it.

    Prompt caching and drafts are Q8Server's, argument for argument, and off by default: submit(..., n_cached=n)
    admits over rows the caller's engine already holds (rama_serve_admit_at), prefix_cache=k keeps k donor engines whose shared
    prefixes are forked into a new request's engine (rama_q8_kv_fork: the KV cache is fp32 in both stacks), and n_draft=K > 0 begins
    the chain with rama_serve_begin_spec: a decoding request's n-gram guesses take the rows of a tile that no slot wants and are
    verified in the same weight pass.  The tokens are the same whatever these are.

    Model drafts.  draft=Q8Model (a small Q8 model over the same vocabulary on the same device --
    Q8Model.from_model makes one from an fp32 Model) with n_draft=K in 1..15 begins the chain with rama_serve_begin_model: the
    guesses are that model's own next tokens under the request's sampler instead of the lookup -- no hint_cap, ngram ignored, at
    most 64 slots.  The server owns one draft engine per slot and prefills it with the request's context before the admission."""

    ABI = "rama_serve"
    NAME = "Server"

    def __init__(self, model: Model, n_slots: int, max_rows=None, max_new_cap: int = 256, n_draft: int = 0, ngram: int = 3,
                 hint_cap: int = 0, prefix_cache: int = 0, draft: Q8Model = None, preempt: bool = False):
        if draft is not None and draft.device is not model.device:
            raise ValueError("Server: the draft model is on another device context")
        super().__init__(model, n_slots, max_rows, max_new_cap, prefix_cache, n_draft, ngram, hint_cap, draft, preempt)

    def _new_engine(self, model=None):
        return Q8Engine(self.device, model) if model is not None else Engine(self.device, self.model)
