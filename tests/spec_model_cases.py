"""The cases of tests/test_hip_q8_spec_model.py: the (target <- draft) pairs of the speculative chain with a draft model, their
shapes, and the inputs chosen so that every accept outcome occurs.  No GPU, nothing of rama_amd imported."""

STORIES15M = dict(dim=288, hidden_dim=768, n_layers=6, n_heads=6, n_kv_heads=6, vocab_size=32000, seq_len=256, shared_weight=True)

# the near-copy pair: one synthetic stories15M-shaped model quantized at two group sizes.  The weights are the same fp32 numbers, so the
# draft's logits are the target's up to quantization noise: greedy it agrees with the target, sampled (T 1) it agrees now and then.
NEAR_SEED = 2
NEAR_GS = (32, 16)                       # (target, draft)

# pair -> (target, draft, (n_context, max_new)).  A name is a fixture under tests/golden; "synth15m/<gs>" is the synthetic model above.
# untied <- untied and gs8 <- gs8 run to the END of their context windows (n_context + max_new == seq_len); untied <- tied to the end
# of the DRAFT's (seq_len 16), which has another dim and group size than the target.  gs8 takes the generic product kernels, and its
# vocabulary (37) is no multiple of 4.
PAIRS = {
    "untied<-untied": ("ckpt_v2_q80_untied", "ckpt_v2_q80_untied", (5, 27)),
    "untied<-tied": ("ckpt_v2_q80_untied", "ckpt_v2_q80_tied", (3, 13)),
    "gs8<-gs8": ("ckpt_v2_q80_gs8", "ckpt_v2_q80_gs8", (4, 20)),
    "synth15m<-near": (f"synth15m/{NEAR_GS[0]}", f"synth15m/{NEAR_GS[1]}", (9, 24)),
}

N_DRAFTS = (1, 2, 7, 15)
SAMPLERS = {"greedy": (0.0, 0.9, 0.0), "sampled": (1.0, 0.9, 0.4)}      # (temperature, topp, u)
# a pair's context: BOS, then default_rng(seed) tokens.  The near-copy pair's (model seed, context seed) were chosen among 5 x 10 candidates
# for a sampled run in which the draft is right once and wrong at the next token: a step with 0 < a < K at every K of the grid but 1.
CONTEXT_SEED = 5
CONTEXT_SEEDS = {"synth15m<-near": 7}    # (every other pair: CONTEXT_SEED)

# THE COVERAGE CONDITION.  Over the (pair, n_draft, sampler) grid above, accepted_hist must be non-zero at 0, at K and at some 0 < a < K.
# A pair of one model with itself accepts everything (a == K on every full step); untied <- tied, two unrelated models, accepts next to
# nothing (a == 0); the partial outcomes come from the near-copy pair.  These are the grid cases in which each outcome was seen when the
# inputs were chosen; test_every_accept_outcome_occurs replays exactly them and fails if an input drifts.
COVERAGE = {
    "none": ("untied<-tied", 7, "greedy"),
    "full": ("untied<-untied", 7, "greedy"),
    "partial": ("synth15m<-near", 7, "sampled"),
}
