"""rama_amd.Server -- continuous batching over an fp32 Model in parity mode (rama_serve_*): the counterpart of
Q8Server without prompt caching and drafts.  Both are rama_amd.q8.ServeLoop -- the queue, the mirror of the slot table, the steps to
the next finish by the host plan, admissions behind the steps in flight, the rings -- over their own entries and engines."""
from __future__ import annotations

from .engine import Engine, Model
from .q8 import ServeLoop, TOPP_U_CPU, serve_plan


class Server(ServeLoop):
    """n_slots sequence slots share parity-mode weight passes of max_rows rows (tiles of 32).  Every request's tokens are those
    Engine.generate gives it alone in parity mode -- the reference's own.  The device context must be in parity mode
    ("ref_order" = 1) and stay there.  One fp32 serving chain per device context; a Q8Server may be live next to it."""

    ABI = "rama_serve"
    NAME = "Server"

    def __init__(self, model: Model, n_slots: int, max_rows=None, max_new_cap: int = 256):
        self._start(model, n_slots, max_rows, max_new_cap)

    def _new_engine(self):
        e = Engine(self.device, self.model)
        self._mine.append(e)
        return e

    def submit(self, context, max_new, temperature=0.0, topp=0.9, u=TOPP_U_CPU, stop_token=None, engine=None):
        """queue a request -> its handle.  It is admitted at once if a slot is free, else when one finishes (step / run).
        engine: the Engine whose run state the sequence uses (default: one the server owns for the slot)."""
        ctx, plan = serve_plan(self.cfg, context, max_new, temperature, topp, u, stop_token, self.max_new_cap, 0, self.NAME)
        h = self._submit(ctx, plan, engine)
        self._admit()
        return h
