"""The Q8 chains' rules restated in plain Python, as oracles for the tests and the benchmarks: the drafting rule, the scheduling
rule with drafts, the accept rule, the tree rules, and whole runs of the speculative chain (n-gram drafts, a tree of them, or a draft model's) and of a serving
chain with drafts replayed from reference tokens.  No library call, nothing of rama_amd imported: rama_amd.q8 imports from here."""
from __future__ import annotations

SERVE_FREE, SERVE_PROMPT, SERVE_DECODE, SERVE_DONE = 0, 1, 2, 3


def _draft_py(hint, seq, n_draft, ngram, room):
    cap = min(n_draft, room)
    if cap <= 0:
        return []
    L = len(seq)
    for n in range(min(ngram, L), 0, -1):
        tail = seq[L - n:]
        for text, hi in ((hint, len(hint)), (seq, L - 1)):          # an occurrence ends at e <= hi: in seq before L
            for e in range(hi, n - 1, -1):
                if text[e - n:e] == tail:
                    return text[e:e + cap]
    return []


def _accept_py(drafts, picks, remaining, stop):
    """the accept rule: picks = Device::sample of rows 0..len(drafts), remaining = the tokens the budget still allows (>= 1) ->
    (drafts accepted, tokens emitted, finished).  The accepted drafts and the pick behind them are emitted, cut at the budget and
    after a stop token."""
    a = 0
    while a < len(drafts) and picks[a] == drafts[a]:
        a += 1
    emit = min(a + 1, remaining)
    fin = emit >= remaining
    for j in range(emit):
        if picks[j] == stop:
            emit, fin = j + 1, True
            break
    return a, emit, fin


def _spec_plan_py(slots, want, max_rows):
    """the scheduling rule with drafts, in Python: slots = [state, n_context, cursor, ...] -> (rows, granted)"""
    nrows = [1 if s[0] in (SERVE_PROMPT, SERVE_DECODE) else 0 for s in slots]
    left = max_rows - sum(nrows)
    for i, s in enumerate(slots):
        if s[0] == SERVE_PROMPT:
            extra = min(s[1] - s[2] - 1, left)
            nrows[i] += extra
            left -= extra
    granted = [0] * len(slots)
    for i, s in enumerate(slots):
        granted[i] = min(want[i], left) if s[0] == SERVE_DECODE else 0
        left -= granted[i]
    rows = []
    for i, s in enumerate(slots):
        for k in range(nrows[i] + granted[i]):
            rows.append((i, s[2] + k, 1 if s[0] == SERVE_DECODE or s[2] + k == s[1] - 1 else 0))
    return rows + [(-1, -1, 0)] * (max_rows - len(rows)), granted


def _cancel_py(cancels, t, slots):
    """the cancel rule: the slots of cancels[t] that are PROMPT or DECODE become DONE before step t, and nothing else changes -> them"""
    hit = []
    for i in sorted(set(int(i) for i in (cancels or {}).get(t, ()))):
        if not 0 <= i < len(slots):
            raise ValueError(f"serve replay: cancels[{t}] names slot {i} of {len(slots)}")
        if slots[i][0] in (SERVE_PROMPT, SERVE_DECODE):
            slots[i][0] = SERVE_DONE
            hit.append(i)
    return hit


def _next_waiting(waiting, reqs, t):
    """the first waiting request that may be admitted before step t (a request's `after_step`, default 0: at once); None: none yet"""
    for q in waiting:
        if reqs[q]["after"] <= t:
            return q
    return None


def spec_replay(ref_tokens, context, hint, n_draft, ngram, max_new, stop_token):
    """the speculative chain's steps as a pure function of its inputs, no library call: ref_tokens = the max_new tokens the
    sequence produces alone (Q8Engine.generate(context[1:], ...)[len(context) - 1:], not cut at the stop token) -> one
    (n_d, a, emitted) per step up to the one that finishes the sequence.  Row j's pick is ref_tokens[emitted so far + j] as long
    as the drafts before it were right, which is all the accept rule looks at."""
    ref, s = [int(t) for t in ref_tokens], [int(t) for t in context]
    hint = [int(t) for t in (hint or [])]
    stop = -1 if stop_token is None else int(stop_token)
    if len(ref) < max_new:
        raise ValueError(f"spec_replay: {len(ref)} reference tokens for max_new {max_new}")
    out, e, fin = [], 0, False
    while not fin:
        remaining = max_new - e
        d = _draft_py(hint, s, n_draft, ngram, remaining - 1)
        picks = ref[e:e + len(d) + 1]
        a, emit, fin = _accept_py(d, picks, remaining, stop)
        s += picks[:emit]
        e += emit
        out.append((len(d), a, emit))
    return out


def spec_tree_draft(hint, seq, n_draft, ngram, room, n_branch, n_rows):
    """the drafting rule over a tree (rama_q8_spec_tree_draft): the continuations of the first n_branch occurrences of the tail
    n-gram -- hint before sequence, larger end first, at the largest n that has any -- inserted in order into a trie whose root
    (node 0) carries seq[-1], until n_rows - 1 nodes exist -> (tok, parent, depth) of nodes 1..m."""
    hint, seq = [int(t) for t in (hint or [])], [int(t) for t in seq]
    cap, L = min(n_draft, room), len(seq)
    tok, parent, depth = [seq[-1]], [-1], [0]
    if cap <= 0:
        return [], [], []
    for n in range(min(ngram, L), 0, -1):
        tail = seq[L - n:]
        occ = [(hint, e) for e in range(len(hint), n - 1, -1) if hint[e - n:e] == tail]
        occ += [(seq, e) for e in range(L - 1, n - 1, -1) if seq[e - n:e] == tail]
        if not occ:
            continue
        full = False
        for text, e in occ[:n_branch]:
            cur = 0
            for t in text[e:e + cap]:
                kids = [j for j in range(1, len(tok)) if parent[j] == cur and tok[j] == t]
                if kids:
                    cur = kids[0]
                    continue
                if len(tok) - 1 >= n_rows - 1:
                    full = True
                    break
                tok.append(t); parent.append(cur); depth.append(depth[cur] + 1)
                cur = len(tok) - 1
            if full:
                break
        break
    return tok[1:], parent[1:], depth[1:]


def spec_tree_accept(tok, parent, picks, remaining, stop):
    """the accept rule over a tree (rama_q8_spec_tree_accept): tok / parent of nodes 1..m, picks of rows 0..m -> (path = the rows
    visited from the root, tokens emitted, finished); a = len(path) - 1."""
    tok, parent = [None] + [int(t) for t in tok], [-1] + [int(t) for t in parent]
    stop = -1 if stop is None else int(stop)
    cur, path, out = 0, [0], [int(picks[0])]
    while out[-1] != stop and len(out) < remaining:
        kids = [j for j in range(1, len(tok)) if parent[j] == cur and tok[j] == out[-1]]
        if not kids:
            break
        cur = kids[0]
        path.append(cur)
        out.append(int(picks[cur]))
    return path, out, len(out) >= remaining or out[-1] == stop


def spec_tree_replay(ref_tokens, context, hint, n_draft, ngram, n_branch, n_rows, max_new, stop_token):
    """the tree chain's steps (rama_q8_spec_begin_tree) as a pure function of its inputs, no library call: ref_tokens as
    spec_replay's -> one (m, a, emitted, off_trunk, off_trunk_deep) per step up to the one that finishes the sequence; off_trunk =
    the accepted nodes with index != depth, off_trunk_deep those of them at depth >= 2.  A node's pick is the reference token
    behind its path as long as the path is right, which is all the accept rule looks at; any other node's pick is never read."""
    ref, s = [int(t) for t in ref_tokens], [int(t) for t in context]
    hint = [int(t) for t in (hint or [])]
    if len(ref) < max_new:
        raise ValueError(f"spec_tree_replay: {len(ref)} reference tokens for max_new {max_new}")
    out, e, fin = [], 0, False
    while not fin:
        remaining = max_new - e
        tok, parent, depth = spec_tree_draft(hint, s, n_draft, ngram, remaining - 1, n_branch, n_rows)
        # a node on the reference's path at depth d is picked ref[e + d]; off it the pick is never compared: -2 matches nothing
        right, picks = [True], [ref[e]]
        for j in range(1, len(tok) + 1):
            ok = right[parent[j - 1]] and e + depth[j - 1] - 1 < len(ref) and tok[j - 1] == ref[e + depth[j - 1] - 1]
            right.append(ok)
            picks.append(ref[e + depth[j - 1]] if ok and e + depth[j - 1] < len(ref) else -2)
        path, emitted, fin = spec_tree_accept(tok, parent, picks, remaining, stop_token)
        off = [j for k, j in enumerate(path) if j != k]
        s += emitted
        e += len(emitted)
        out.append((len(tok), len(path) - 1, len(emitted), len(off), sum(1 for j in off if depth[j - 1] >= 2)))
    return out


def spec_model_replay(ref_tokens, draft_fn, context, n_draft, max_new, stop_token):
    """the steps of the speculative chain with a draft model (rama_q8_spec_begin_model) as a pure function of its inputs, no library
    call: ref_tokens as spec_replay's; draft_fn(prefix, n) = the n tokens the draft model produces alone after the token list prefix,
    under the plan's sampler -> (one (n_d, a, emitted, catch_up) per step up to the one that finishes the sequence, the final draft
    cursor).  n_d = min(n_draft, remaining - 1) (n_context + max_new <= seq_len: the budget binds first); catch_up = the catch-up
    rows the step feeds the draft model: 1 when the draft cursor is one behind the position fed next and the step drafts at all.
    The draft cursor Dc: rows 0..Dc-1 of the draft cache belong to the sequence; P - Dc is 0 or 1 when a step opens."""
    ref, s = [int(t) for t in ref_tokens], [int(t) for t in context]
    stop = -1 if stop_token is None else int(stop_token)
    if len(ref) < max_new:
        raise ValueError(f"spec_model_replay: {len(ref)} reference tokens for max_new {max_new}")
    out, e, fin, cursor = [], 0, False, len(s) - 1
    while not fin:
        L, remaining = len(s), max_new - e
        n_d = max(min(n_draft, remaining - 1), 0)
        gap = L - 1 - cursor
        if gap not in (0, 1):
            raise AssertionError(f"spec_model_replay: the draft cursor {cursor} is {gap} rows behind position {L - 1}")
        d = [int(t) for t in draft_fn(list(s), n_d)] if n_d else []
        if len(d) != n_d:
            raise ValueError(f"spec_model_replay: draft_fn gave {len(d)} tokens for {n_d}")
        picks = ref[e:e + n_d + 1]
        a, emit, fin = _accept_py(d, picks, remaining, stop)
        s += picks[:emit]
        e += emit
        if n_d:                                                    # rows P..P + n_d - 1 carry s[P], d[0..n_d - 1); d[0..a) are part of s now
            cursor = min(L + min(a, n_d - 1), len(s))
        out.append((n_d, a, emit, gap if n_d else 0))
    return out, cursor


def spec_model_tree_shape(cap, n_branch, n_rows):
    """the static shape of a draft model's tree (rama_q8_spec_model_tree_shape): the trunk 1..min(cap, n_rows - 1) first, then level
    by level every node of the level above in ascending index -- a trunk node (index == depth, the root included) gets side children
    of ranks 1..n_branch - 1, any other node one child of rank 0 -- until n_rows - 1 nodes exist -> (parent, depth, rank) of nodes 1..m."""
    parent, depth, rank = [-1], [0], [0]
    for d in range(1, cap + 1):
        if len(parent) - 1 >= n_rows - 1:
            break
        parent.append(d - 1); depth.append(d); rank.append(0)
    for d in range(1, cap + 1):
        for p in range(len(parent)):
            if depth[p] != d - 1:
                continue
            kids = range(1, n_branch) if p == depth[p] else (0,)
            for r in kids:
                if len(parent) - 1 >= n_rows - 1:
                    break
                parent.append(p); depth.append(d); rank.append(r)
    return parent[1:], depth[1:], rank[1:]


def spec_model_tree_candidates(logits, rank0_token, n):
    """the tokens of ranks 1..n of a logits row (rama_q8_spec_model_tree_candidates): all tokens by descending 64-bit key -- high word
    the float32's bits mapped monotonically to unsigned (a NaN where its bits put it), low word the token index --, rank 0's token
    dropped, the first n."""
    import struct
    keys = []
    for i, v in enumerate(logits):
        bits = struct.unpack("<I", struct.pack("<f", v))[0]
        hi = bits ^ (0xFFFFFFFF if bits >> 31 else 0x80000000)
        if i != int(rank0_token):
            keys.append((hi << 32) | i)
    keys.sort(reverse=True)
    return [k & 0xFFFFFFFF for k in keys[:n]]


def spec_model_tree_replay(ref_tokens, logits_fn, context, n_draft, n_branch, n_rows, max_new, stop_token, sampler):
    """the steps of the speculative chain with a draft model's tree (rama_q8_spec_begin_model_tree) as a pure function of its inputs,
    no library call: ref_tokens as spec_replay's; logits_fn(prefix) = the draft model's logits row after the token list prefix;
    sampler(row) = Device::sample of a logits row under the plan's sampler (rank 0) -> (one (cap, tok, parent, depth, picks, a, path,
    emitted, catch_up) per step up to the one that finishes the sequence -- tok / parent / depth / picks of nodes 0..m, a pick that is
    never compared given as -2 --, (the final cursor, the final draft cursor)).  cap = min(n_draft, remaining - 1) (n_context +
    max_new <= seq_len: the budget binds first).  A node's token: rank 0 = sampler of the row after the prefix and the path to its
    parent, rank r >= 1 = spec_model_tree_candidates of that row behind rank 0's token."""
    ref, s = [int(t) for t in ref_tokens], [int(t) for t in context]
    if len(ref) < max_new:
        raise ValueError(f"spec_model_tree_replay: {len(ref)} reference tokens for max_new {max_new}")
    out, e, fin, cursor = [], 0, False, len(s) - 1
    while not fin:
        L, remaining = len(s), max_new - e
        cap = max(min(n_draft, remaining - 1), 0)
        gap = L - 1 - cursor
        if gap not in (0, 1):
            raise AssertionError(f"spec_model_tree_replay: the draft cursor {cursor} is {gap} rows behind position {L - 1}")
        par, dep, rank = spec_model_tree_shape(cap, n_branch, n_rows)
        parent, depth, rank = [-1] + par, [0] + dep, [0] + rank
        tok, rows = [s[-1]], {}
        for j in range(1, len(parent)):
            p = parent[j]
            if p not in rows:                                      # the row of the pass that feeds p: its first choice, then the next ones
                chain, c = [], p
                while c > 0:
                    chain.append(tok[c])
                    c = parent[c]
                row = logits_fn(list(s) + chain[::-1])
                first = int(sampler(row))
                rows[p] = [first] + spec_model_tree_candidates(row, first, n_branch - 1)
            tok.append(int(rows[p][rank[j]]))
        right, picks = [True], [ref[e]]
        for j in range(1, len(tok)):
            ok = right[parent[j]] and e + depth[j] - 1 < len(ref) and tok[j] == ref[e + depth[j] - 1]
            right.append(ok)
            picks.append(ref[e + depth[j]] if ok and e + depth[j] < len(ref) else -2)
        path, emitted, fin = spec_tree_accept(tok[1:], parent[1:], picks, remaining, stop_token)
        a = len(path) - 1
        s += emitted
        e += len(emitted)
        if cap:                                                    # the fed nodes of the path, depths 1..min(a, cap - 1), are part of s now
            cursor = min(L + min(a, cap - 1), len(s))
        out.append((cap, tok, parent, depth, picks, a, path, emitted, gap if cap else 0))
    return out, (len(s) - 1, cursor)


def serve_spec_replay(requests, ref_tokens, n_slots, max_rows, use_slots=None, cancels=None):
    """a whole workload of a serving chain with drafts as a pure function of its inputs, no library call.  requests = dicts with
    context and max_new, and optionally stop_token, n_draft (0), ngram (3), hint and n_cached (0); ref_tokens[i] = the max_new
    tokens request i produces alone (Q8Engine.generate(context[1:], ...)[len(context) - 1:], not cut at the stop token).
    Admission: before every step the waiting requests, in order, take the slots of use_slots (default: all) that are FREE or
    DONE, in ascending slot index.  Every step is the draft rule per DECODE slot, the scheduling rule, and the accept rule by
    comparison with the reference tokens: row j's pick is ref[n_out + j] as long as the drafts before it were right, which is
    all the accept rule looks at.  -> dict(steps = one dict per step: admitted [(slot, request)], rows, want, granted, accepted
    {slot: a} for the DECODE slots, emitted {slot: n}, finished [slots]; counters = what rama_q8_serve_spec_stats reports;
    finish_step = per request the step it finishes in; slot = per request its slot; outputs = per request its tokens).
    cancels = {step: [slots]}: before step `step` (and before its admissions) the slots named that are PROMPT or DECODE become
    DONE, and nothing else changes -- the rule of rama_q8_serve_cancel.  A request may carry after_step: it is not admitted
    before that step (a continuation of a cancelled request: context ++ outputs, n_cached = the cursor, the budget left, the
    reference tokens from there on).  With cancels given, each step dict has cancelled = the slots a cancel ended before it, the result
    cancelled_at = per request the step before which it was cancelled (None: it was not); a cancelled request has no
    finish_step."""
    reqs = []
    for r, ref in zip(requests, ref_tokens):
        ctx, new = [int(t) for t in r["context"]], int(r["max_new"])
        if len(ref) < new:
            raise ValueError(f"serve_spec_replay: {len(ref)} reference tokens for max_new {new}")
        stop = r.get("stop_token")
        reqs.append(dict(ctx=ctx, new=new, stop=-1 if stop is None else int(stop), K=int(r.get("n_draft", 0)), N=int(r.get("ngram", 3)),
                         hint=[int(t) for t in (r.get("hint") or [])], cached=int(r.get("n_cached", 0)), ref=[int(t) for t in ref],
                         after=int(r.get("after_step", 0))))
    usable = list(range(n_slots)) if use_slots is None else sorted(use_slots)
    slots = [[SERVE_FREE, 0, 0, 0, 0] for _ in range(n_slots)]      # state, n_context, cursor, n_out, max_new
    who, text = [None] * n_slots, [None] * n_slots
    waiting = list(range(len(reqs)))
    steps, finish, slot_of, outputs = [], [None] * len(reqs), [None] * len(reqs), [[] for _ in reqs]
    cancelled_at = [None] * len(reqs)
    cnt = dict(steps=0, rows_decode=0, rows_draft=0, rows_prompt=0, rows_idle=0, drafts_wanted=0, drafts_granted=0, drafts_accepted=0,
               tokens_emitted=0, accepted_hist=[0] * 16)
    while waiting or any(s[0] in (SERVE_PROMPT, SERVE_DECODE) for s in slots):
        t = len(steps)
        cancelled = _cancel_py(cancels, t, slots)
        for i in cancelled:
            cancelled_at[who[i]] = t
        admitted = []
        for i in usable:
            q = _next_waiting(waiting, reqs, t)
            if q is not None and slots[i][0] in (SERVE_FREE, SERVE_DONE):
                waiting.remove(q)
                r = reqs[q]
                slots[i] = [SERVE_PROMPT, len(r["ctx"]), r["cached"], 0, r["new"]]
                who[i], text[i], slot_of[q] = q, list(r["ctx"]), i
                admitted.append((i, q))
        if not any(s[0] in (SERVE_PROMPT, SERVE_DECODE) for s in slots):
            if not waiting:
                break                                              # (a cancel ended the last live slot)
            if all(reqs[q]["after"] <= t for q in waiting):
                raise ValueError("serve_spec_replay: requests are waiting but no slot can take them")
        want, drafts = [0] * n_slots, [[] for _ in range(n_slots)]
        for i, s in enumerate(slots):
            if s[0] == SERVE_DECODE and reqs[who[i]]["K"] > 0:
                r = reqs[who[i]]
                drafts[i] = _draft_py(r["hint"], text[i], r["K"], r["N"], s[4] - s[3] - 1)      # (n_context + max_new <= seq_len: the budget binds first)
                want[i] = len(drafts[i])
        rows, granted = _spec_plan_py(slots, want, max_rows)
        used = sum(1 for r in rows if r[0] >= 0)
        n_dec = sum(1 for s in slots if s[0] == SERVE_DECODE)
        cnt["steps"] += 1
        cnt["rows_decode"] += n_dec
        cnt["rows_draft"] += sum(granted)
        cnt["rows_prompt"] += used - n_dec - sum(granted)
        cnt["rows_idle"] += max_rows - used
        cnt["drafts_wanted"] += sum(want)
        accepted, emitted, finished = {}, {}, []
        for i, s in enumerate(slots):
            n = sum(1 for r in rows if r[0] == i)
            if n == 0:
                continue
            r = reqs[who[i]]
            if s[0] == SERVE_PROMPT and s[2] + n < s[1]:
                s[2] += n
                continue
            if s[0] == SERVE_PROMPT:
                picks, emit = r["ref"][:1], 1
                fin = s[4] <= 1 or picks[0] == r["stop"]
                s[2] = s[1]
            else:
                d = drafts[i][:granted[i]]
                picks = r["ref"][s[3]:s[3] + len(d) + 1]
                a, emit, fin = _accept_py(d, picks, s[4] - s[3], r["stop"])
                accepted[i] = a
                cnt["drafts_granted"] += len(d)
                cnt["drafts_accepted"] += a
                cnt["accepted_hist"][a] += 1
                s[2] += emit
            emitted[i] = emit
            cnt["tokens_emitted"] += emit
            text[i] += picks[:emit]
            outputs[who[i]] += picks[:emit]
            s[3] += emit
            s[0] = SERVE_DONE if fin else SERVE_DECODE
            if fin:
                finished.append(i)
                finish[who[i]] = len(steps)
        steps.append(dict(admitted=admitted, rows=rows, want=want, granted=granted, accepted=accepted, emitted=emitted, finished=finished,
                          slots=[tuple(s) for s in slots]))
        if cancels is not None:
            steps[-1]["cancelled"] = cancelled
    out = dict(steps=steps, counters=cnt, finish_step=finish, slot=slot_of, outputs=outputs)
    if cancels is not None:
        out["cancelled_at"] = cancelled_at
    return out


def serve_replay(requests, ref_tokens, n_slots, max_rows, use_slots=None, cancels=None):
    """a whole workload of a serving chain WITHOUT drafts (rama_q8_serve_begin, rama_serve_begin) as a pure function of its inputs:
    serve_spec_replay with no slot drafting -- the scheduling rule with drafts is the plain rule when nobody wants one --, so one
    cancel schedule replays on all three kinds of chain.  -> serve_spec_replay's dict without the drafting entries: counters =
    what rama_q8_serve_stats reports (steps, rows_decode, rows_prompt, rows_idle)."""
    plain = [{k: v for k, v in r.items() if k not in ("n_draft", "ngram", "hint")} for r in requests]
    out = serve_spec_replay(plain, ref_tokens, n_slots, max_rows, use_slots, cancels or {})
    out["counters"] = {k: out["counters"][k] for k in ("steps", "rows_decode", "rows_prompt", "rows_idle")}
    for st in out["steps"]:
        for k in ("want", "granted", "accepted"):
            del st[k]
    return out


def serve_model_replay(requests, ref_tokens, draft_fn, n_slots, max_rows, use_slots=None, cancels=None):
    """a whole workload of a serving chain with a draft model (rama_q8_serve_begin_model) as a pure function of its inputs, no library
    call.  requests and ref_tokens as serve_spec_replay's (n_draft: the drafts per step of the request, 0: none; ngram and hint do not
    exist here); draft_fn(prefix, n) = the n tokens the draft model produces alone after the token list prefix under the request's
    sampler -- one callable, or one per request.  Admission as serve_spec_replay's.  Every step: a DECODE slot with n_draft > 0 wants
    min(n_draft, max_new - n_out - 1) (n_context + max_new <= seq_len: the budget binds first) and feeds the draft model s[Dc..P]
    whatever it is granted; the scheduling rule; the granted drafts d = draft_fn(s, g); the accept rule against the reference tokens;
    Dc' = min(L + min(a, max(g - 1, 0)), new L).  -> serve_spec_replay's dict, and besides: per step `drafting` = {slot: (g, a,
    emitted, catch_up)} for the slots that fed the draft model and `cursors` = every slot's draft cursor after the step; counters
    also has draft_passes, draft_rows_fed and catch_up_rows (rama_q8_serve_model_stats); cursor = per request its final draft cursor.
    cancels and a request's after_step: as serve_spec_replay's; a cancelled slot's draft cursor stays where it is."""
    fns = list(draft_fn) if isinstance(draft_fn, (list, tuple)) else [draft_fn] * len(requests)
    reqs = []
    for r, ref in zip(requests, ref_tokens):
        ctx, new = [int(t) for t in r["context"]], int(r["max_new"])
        if len(ref) < new:
            raise ValueError(f"serve_model_replay: {len(ref)} reference tokens for max_new {new}")
        stop = r.get("stop_token")
        reqs.append(dict(ctx=ctx, new=new, stop=-1 if stop is None else int(stop), K=int(r.get("n_draft", 0)), cached=int(r.get("n_cached", 0)),
                         ref=[int(t) for t in ref], after=int(r.get("after_step", 0))))
    usable = list(range(n_slots)) if use_slots is None else sorted(use_slots)
    slots = [[SERVE_FREE, 0, 0, 0, 0] for _ in range(n_slots)]      # state, n_context, cursor, n_out, max_new
    who, text, Dc = [None] * n_slots, [None] * n_slots, [0] * n_slots
    waiting = list(range(len(reqs)))
    steps, finish, slot_of, outputs, final = [], [None] * len(reqs), [None] * len(reqs), [[] for _ in reqs], [None] * len(reqs)
    cancelled_at = [None] * len(reqs)
    cnt = dict(steps=0, rows_decode=0, rows_draft=0, rows_prompt=0, rows_idle=0, drafts_wanted=0, drafts_granted=0, drafts_accepted=0,
               tokens_emitted=0, accepted_hist=[0] * 16, draft_passes=0, draft_rows_fed=0, catch_up_rows=0)
    while waiting or any(s[0] in (SERVE_PROMPT, SERVE_DECODE) for s in slots):
        t = len(steps)
        cancelled = _cancel_py(cancels, t, slots)
        for i in cancelled:
            cancelled_at[who[i]] = t
        admitted = []
        for i in usable:
            q = _next_waiting(waiting, reqs, t)
            if q is not None and slots[i][0] in (SERVE_FREE, SERVE_DONE):
                waiting.remove(q)
                r = reqs[q]
                slots[i] = [SERVE_PROMPT, len(r["ctx"]), r["cached"], 0, r["new"]]
                who[i], text[i], slot_of[q], Dc[i] = q, list(r["ctx"]), i, len(r["ctx"])
                admitted.append((i, q))
        if not any(s[0] in (SERVE_PROMPT, SERVE_DECODE) for s in slots):
            if not waiting:
                break                                              # (a cancel ended the last live slot)
            if all(reqs[q]["after"] <= t for q in waiting):
                raise ValueError("serve_model_replay: requests are waiting but no slot can take them")
        want, gap = [0] * n_slots, {}
        for i, s in enumerate(slots):
            if s[0] == SERVE_DECODE and reqs[who[i]]["K"] > 0:
                want[i] = max(min(reqs[who[i]]["K"], s[4] - s[3] - 1), 0)
                gap[i] = s[2] - Dc[i]
                if gap[i] not in (0, 1):
                    raise AssertionError(f"serve_model_replay: slot {i}'s draft cursor {Dc[i]} is {gap[i]} rows behind position {s[2]}")
        rows, granted = _spec_plan_py(slots, want, max_rows)
        used = sum(1 for r in rows if r[0] >= 0)
        n_dec = sum(1 for s in slots if s[0] == SERVE_DECODE)
        cnt["steps"] += 1
        cnt["rows_decode"] += n_dec
        cnt["rows_draft"] += sum(granted)
        cnt["rows_prompt"] += used - n_dec - sum(granted)
        cnt["rows_idle"] += max_rows - used
        cnt["drafts_wanted"] += sum(want)
        accepted, emitted, finished, drafting = {}, {}, [], {}
        for i, s in enumerate(slots):
            n = sum(1 for r in rows if r[0] == i)
            if n == 0:
                continue
            r = reqs[who[i]]
            if s[0] == SERVE_PROMPT and s[2] + n < s[1]:
                s[2] += n
                continue
            if s[0] == SERVE_PROMPT:
                picks, emit = r["ref"][:1], 1
                fin = s[4] <= 1 or picks[0] == r["stop"]
                s[2] = s[1]
            else:
                g, L = granted[i], len(text[i])
                d = [int(t) for t in fns[who[i]](list(text[i]), g)] if g else []
                if len(d) != g:
                    raise ValueError(f"serve_model_replay: draft_fn gave {len(d)} tokens for {g}")
                picks = r["ref"][s[3]:s[3] + g + 1]
                a, emit, fin = _accept_py(d, picks, s[4] - s[3], r["stop"])
                accepted[i] = a
                cnt["drafts_granted"] += g
                cnt["drafts_accepted"] += a
                cnt["accepted_hist"][a] += 1
                s[2] += emit
                if i in gap:
                    Dc[i] = min(L + min(a, max(g - 1, 0)), L + emit)
                    drafting[i] = (g, a, emit, gap[i])
                    cnt["draft_passes"] += max(g, 1)
                    cnt["draft_rows_fed"] += gap[i] + max(g, 1)
                    cnt["catch_up_rows"] += gap[i]
            emitted[i] = emit
            cnt["tokens_emitted"] += emit
            text[i] += picks[:emit]
            outputs[who[i]] += picks[:emit]
            s[3] += emit
            s[0] = SERVE_DONE if fin else SERVE_DECODE
            final[who[i]] = Dc[i]
            if fin:
                finished.append(i)
                finish[who[i]] = len(steps)
        steps.append(dict(admitted=admitted, rows=rows, want=want, granted=granted, accepted=accepted, emitted=emitted, finished=finished,
                          slots=[tuple(s) for s in slots], drafting=drafting, cursors=list(Dc)))
        if cancels is not None:
            steps[-1]["cancelled"] = cancelled
    out = dict(steps=steps, counters=cnt, finish_step=finish, slot=slot_of, outputs=outputs, cursor=final)
    if cancels is not None:
        out["cancelled_at"] = cancelled_at
    return out
