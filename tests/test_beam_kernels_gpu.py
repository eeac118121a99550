"""The beam-search kernels (csrc/beam.hip) at kernel level, model-free, against the host restatement of
tests/beam_refs.py (pinned to transformers by test_beam_refs_cpu.py).

- direct-table scenarios: the row tables are written by hand (m = 0, ls = 0, dyadic "log-probabilities"), so every
  score is exact fp32 arithmetic; after every icap_beam_update the whole live workspace is compared. The scripts
  force the branches listed in FORCED, and test_scripts_force_every_branch (no GPU) asserts that they do.
- capacity and bounds: W * max_len = 1024 with T = 1024 over 128 scripted reorders; pos + 1 == T with guard words
  round the workspace.
- through BeamState.step (rowtop, then update) on random, heavily tied logits.
- icap_beam_rowtop's edges: V round the 256-thread stride and below K, padding columns that must not win, ties."""

import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import beam_refs as BR

D = 8
P0 = 3  # prefix positions of the direct scenarios; n_positions = P0 + 2, so wpe clamps from step 2 on

# name: W, lp, dtype, V, max_len, steps run (< max_len: the loop is stopped before the budget), eos, seed
SCENARIOS = {
    "w1": dict(W=1, lp=0.0, dt=torch.float32, V=16, L=6, steps=6, eos=5, seed=2),
    "w2": dict(W=2, lp=0.0, dt=torch.bfloat16, V=24, L=8, steps=8, eos=23, seed=2),
    "w3_lp2": dict(W=3, lp=2.0, dt=torch.float32, V=40, L=8, steps=8, eos=0, seed=3),
    "w4": dict(W=4, lp=0.0, dt=torch.bfloat16, V=64, L=10, steps=10, eos=17, seed=4),
    "w4_lp075_cut": dict(W=4, lp=0.75, dt=torch.float32, V=33, L=10, steps=6, eos=32, seed=5),
    "w5": dict(W=5, lp=0.0, dt=torch.float32, V=48, L=8, steps=8, eos=9, seed=6),
    "w8_lp2": dict(W=8, lp=2.0, dt=torch.bfloat16, V=64, L=9, steps=9, eos=31, seed=7),
    "w8_cut": dict(W=8, lp=0.0, dt=torch.float32, V=20, L=7, steps=5, eos=3, seed=8),
}
FORCED = ("cross_beam_tie", "same_beam_tie", "hit_below_W", "hit_from_W_up_unrecorded", "W_hits_before_budget",
          "more_than_W_hits", "evicts_kept", "new_equals_kept", "two_new_equal", "early_done", "hit_after_done",
          "better_hit_after_done", "budget_step", "no_finished_at_finalize", "x_null", "wpe_clamp")


# ---------------------------------------------------------------------------------------------- scripts (host)
def _row(entries, K, V, eos, rng):
    """A row table of K (value, token) pairs: `entries` first, then fillers far below, in rowtop's order
    (descending, ties -> lower token)."""
    used = {t for _, t in entries}
    free = [t for t in range(V) if t not in used and t != eos]
    rng.shuffle(free)
    low = min([v for v, _ in entries], default=0.0)
    rows = list(entries) + [(low - 16.0 - k, free[k]) for k in range(K - len(entries))]
    return sorted(rows, key=lambda e: (-e[0], e[1]))


def _random_row(K, V, eos, rng, quantum, p_eos):
    toks = [t for t in rng.permutation(V).tolist() if t != eos][:K]
    vals = (-quantum * rng.integers(0, 7, size=K)).tolist()
    ent = list(zip(vals, toks))
    if rng.random() < p_eos:
        ent[int(rng.integers(0, K))] = (-quantum * int(rng.integers(0, 4)), eos)
    return sorted(ent, key=lambda e: (-e[0], e[1]))


def _tables(rows):
    return (np.array([[v for v, _ in r] for r in rows], dtype=np.float32),
            np.array([[t for _, t in r] for r in rows], dtype=np.int32))


@functools.lru_cache(maxsize=None)
def run_script(name):
    """The scenario played on the restatement: [(top_val, top_idx, step, pos, x_is_null, infos, state after)].
    Caption 0 fills its finished list at step 1 and is done, then keeps meeting EOS on top of its running beams;
    caption 1 meets EOS at random ranks among coarse, heavily tied scores; caption 2 never meets EOS."""
    s = SCENARIOS[name]
    W, V, L, eos = s["W"], s["V"], s["L"], s["eos"]
    K = 8 if W <= 4 else 16
    rng = np.random.default_rng(s["seed"])
    quantum = 0.5 if s["lp"] == 0.0 else 0.25
    ref = BR.BeamRef(3, W, V, L, P0 + L, eos, s["lp"], K)
    ref.init(P0)
    out = []
    for step in range(s["steps"]):
        rows = []
        for i in range(W):  # caption 0
            toks = [t for t in rng.permutation(V).tolist() if t != eos][:K]
            if step == 0:
                rows.append(_row([(-k / 8.0, toks[k]) for k in range(K)], K, V, eos, rng))
            elif step == 1:
                rows.append(_row([(0.0, eos)] + [(-1.0 - k / 4.0, toks[k]) for k in range(K - 1)], K, V, eos, rng))
            else:
                rows.append(_row([(0.0, eos)] + [(-(k + 1) / 4.0, toks[k]) for k in range(K - 1)], K, V, eos, rng))
        rows += [_random_row(K, V, eos, rng, quantum, 0.5) for _ in range(W)]   # caption 1
        rows += [_random_row(K, V, eos, rng, quantum, 0.0) for _ in range(W)]   # caption 2
        val, idx = _tables(rows)
        pos = P0 + step - 1
        x_null = step == 2 or step == s["steps"] - 1
        z = np.zeros(3 * W, dtype=np.float32)
        infos = ref.update(val, idx, z, z, step, pos)
        out.append((val, idx, step, pos, x_null, infos, copy.deepcopy(ref)))
    assert not ref.fragile_comparisons(), (name, ref.fragile_comparisons()[:3])
    return out


def forced_branches(name):
    """Which of FORCED the scenario's script really runs, judged on the host from the restatement's decisions."""
    s = SCENARIOS[name]
    W, V, L = s["W"], s["V"], s["L"]
    got = set()
    done_at = {}
    steps = run_script(name)
    for val, idx, step, pos, x_null, infos, ref in steps:
        n = step + 1
        if x_null:
            got.add("x_null")
        if pos + 1 > P0 + 1:
            got.add("wpe_clamp")
        for b, info in enumerate(infos):
            cs = info["cands"] + ([(info["boundary"][0], info["boundary"][1] // V, -1)] if info["boundary"] else [])
            for a, c in zip(cs[:-1], cs[1:]):
                if a[0] == c[0]:
                    got.add("same_beam_tie" if a[1] == c[1] else "cross_beam_tie")
            hits, live = info["hits"], not info["was_done"]
            if n == L:
                got.add("budget_step")
                if sum(hits) > W:
                    got.add("more_than_W_hits")
            elif sum(hits) == W and W > 1:
                got.add("W_hits_before_budget")
            if live and any(hits[:W]):
                got.add("hit_below_W")
            worst = ref.fin_score[b, W - 1] if ref.fin_cnt[b] == W else -np.inf
            for j in range(W, 2 * W):  # a hit past the first W that would enter the list if it were scanned
                if live and hits[j] and n < L and ref._norm(np.float32(info["cands"][j][0]), n)[0] > worst:
                    got.add("hit_from_W_up_unrecorded")
            if info["evicted_kept"] and any(new for new, _ in info["merged"]):
                got.add("evicts_kept")
            ent = info["entries"]
            kept_in = {src for new, src in info["merged"] if not new}
            for new, src, sc in ent:
                if not new:
                    continue
                if s["lp"] == 0.0 and any(not n2 and s2 == sc and k2 in kept_in for n2, k2, s2 in ent):
                    got.add("new_equals_kept")
                if (True, src) in info["merged"] and any(n2 and k2 != src and s2 == sc for n2, k2, s2 in ent):
                    got.add("two_new_equal")
            if info["done_now"]:
                done_at[b] = step
            if info["was_done"] and any(hits[:W]) and n < L:
                got.add("hit_after_done")
                if any(hits[j] and ref._norm(np.float32(info["cands"][j][0]), n)[0] > ref.fin_score[b, W - 1]
                       for j in range(W)):
                    got.add("better_hit_after_done")
    last = steps[-1][6]
    if 0 in done_at and all(done_at.get(b, s["steps"]) >= done_at[0] + 3 for b in (1, 2)):
        # its finished list is frozen from then on while its running beams move
        frozen = [(r.fin_score[0].tobytes(), r.fin_seq[0].tobytes(), r.fin_len[0].tobytes())
                  for *_, r in steps[done_at[0]:]]
        moving = {r.run_seq[0].tobytes() for *_, r in steps[done_at[0]:]}
        if len(set(frozen)) == 1 and len(moving) == len(frozen):
            got.add("early_done")
    if s["steps"] < L and (last.fin_cnt == 0).any():
        out, n = last.finalize()
        b = int(np.nonzero(last.fin_cnt == 0)[0][0])
        assert n[b] == L and np.array_equal(out[b], last.run_seq[b, 0])
        got.add("no_finished_at_finalize")
    return got


def test_scripts_force_every_branch():
    """No GPU: every scenario's script forces what it is there for, and together they force all of FORCED."""
    got = {name: forced_branches(name) for name in SCENARIOS}
    union = set().union(*got.values())
    assert union == set(FORCED), set(FORCED) - union
    for name, s in SCENARIOS.items():
        need = {"cross_beam_tie" if s["W"] > 1 else "same_beam_tie", "same_beam_tie", "hit_below_W",
                "hit_after_done", "x_null", "wpe_clamp"}
        need |= {"early_done"} if s["W"] >= 3 else set()  # narrower lists fill within a step or two everywhere
        need |= {"no_finished_at_finalize"} if s["steps"] < s["L"] else {"budget_step", "more_than_W_hits"}
        assert need <= got[name], (name, need - got[name])
    assert "better_hit_after_done" in got["w3_lp2"] and "better_hit_after_done" in got["w8_lp2"]
    assert {"new_equals_kept", "two_new_equal", "evicts_kept", "hit_from_W_up_unrecorded"} <= got["w4"]


# ---------------------------------------------------------------------------------------------- device driving
def _state(dev, B, W, V, L, T, eos, lp, dt, n_pos, seed=0):
    from icap import ops

    g = torch.Generator().manual_seed(100 + seed)
    wte = torch.randn((V, D), generator=g).to(dt)
    wpe = torch.randn((n_pos, D), generator=g).to(dt)
    st = ops.BeamState(B, W, V, L, T, eos, lp, dev)
    st.wte, st.wpe = wte.to(dev), wpe.to(dev)  # keep the device copies alive
    st.set_embedding(dt, D, n_pos, st.wte, st.wpe, None)
    st.x = torch.full((B * W, D), 77.0, dtype=dt, device=dev)
    st.offs = ops.beam_layout(B, W, T, L)
    return st, wte, wpe


def _update(st, val, idx, m, ls, step, pos, x):
    from icap._lib import call
    from icap.ops import _p, _stream

    st.top_val.copy_(torch.from_numpy(val))
    st.top_idx.copy_(torch.from_numpy(idx))
    st.top_m.copy_(torch.from_numpy(m))
    st.top_ls.copy_(torch.from_numpy(ls))
    st.args.x = _p(x)
    call("icap_beam_update", C.byref(st.args), step, pos, _stream())


def _read(st, ws=None):
    a = st.args
    w = (st.ws if ws is None else ws).cpu().numpy()
    return BR.split_workspace(w, st.offs, a.B, a.W, a.T, a.max_len)


def _check_final(st, ref):
    out, n = st.finalize()
    eo, en = ref.finalize()
    assert np.array_equal(n.cpu().numpy(), en), (n, en)
    assert np.array_equal(out.cpu().numpy(), eo), (out, eo)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_beam_update_direct_tables(dev, name):
    """icap_beam_init / icap_beam_update / icap_beam_finalize on hand-written row tables: after every step every
    live workspace field equals the restatement (ints and run_score bitwise, fin_score bitwise at lp = 0 and within
    4 fp32 ulp of the fp64 quotient otherwise), x equals wte[token] + wpe[clamped position] bitwise (and is left
    alone when x = NULL), and finalize returns the restatement's ids and lengths."""
    s = SCENARIOS[name]
    W, L = s["W"], s["L"]
    st, wte, wpe = _state(dev, 3, W, s["V"], L, P0 + L, s["eos"], s["lp"], s["dt"], P0 + 2, s["seed"])
    st.init(P0)
    z = np.zeros(3 * W, dtype=np.float32)
    x_before = st.x.clone()
    for val, idx, step, pos, x_null, infos, ref in run_script(name):
        _update(st, val, idx, z, z, step, pos, None if x_null else st.x)
        BR.assert_state_equal(ref, _read(st), step, pos, tag=name)
        if x_null:
            assert torch.equal(st.x, x_before), (name, step, "x written though NULL was passed")
        else:
            exp = ref.next_x(wte, wpe, pos, s["dt"])
            assert torch.equal(st.x.cpu().view(torch.int16 if s["dt"] == torch.bfloat16 else torch.int32),
                               exp.view(torch.int16 if s["dt"] == torch.bfloat16 else torch.int32)), (name, step)
            x_before = st.x.clone()
    _check_final(st, ref)


# ---------------------------------------------------------------------------------------------- capacity, bounds
def _parent_tables(ref, step, parents_of, V, eos):
    """Row tables that make caption b's new beam i descend from parents_of(b)[i]: new beam i gets the score
    base - i / 4 with base below every running score, every other entry lies 16 and more below that."""
    W, K = ref.W, ref.K
    rows = []
    for b in range(ref.B):
        parents = parents_of(b)
        rs = ref.run_score[b].astype(np.float64)
        live = rs[rs > -1e8]
        base = float(live.min()) - 1.0
        for p in range(W):
            if rs[p] <= -1e8:  # step 0: beams 1.. are impossible whatever their row says
                ent = []
            else:
                ent = [(base - i / 4.0 - rs[p], (step * 3 + 5 * i + b) % (V - 1)) for i in range(W) if parents[i] == p]
            used = {t for _, t in ent}
            free = [t for t in range(V) if t not in used and t != eos]
            low = min([v for v, _ in ent], default=0.0)
            rows.append(ent + [(low - 16.0 - k, free[k]) for k in range(K - len(ent))])
    return _tables(rows)


def _scripted_parents(step, W, b):
    if step == 0:
        return [0] * W
    kind = (step + b) % 4
    if kind == 0:
        return [W - 1] * W                                  # every beam descends from the last one
    if kind == 1:
        return [(i + 1) % W for i in range(W)]              # cyclic shift
    if kind == 2:
        return [(i * 3 + step) % W for i in range(W)]       # a permutation (W = 8) that moves with the step
    return [i // 2 for i in range(W)]                       # pairs share a parent


def _run_reorders(dev, B, W, V, L, P, T, guard, anc_every):
    from icap import ops

    eos = V - 1
    st, wte, wpe = _state(dev, B, W, V, L, T, eos, 0.0, torch.float32, 16)
    SENT = 0x5A5A5A5A
    if guard:  # the workspace as a 16-byte-aligned view inside a larger tensor, guard words on both sides
        n = st.ws.numel()
        big = torch.full((guard + n + guard,), SENT, dtype=torch.int32, device=dev)
        ws = big[guard: guard + n]
        assert ws.data_ptr() % 16 == 0
        st.args.ws = ws.data_ptr()
        st.done = ws[st.offs["done"]: st.offs["done"] + B]
    else:
        big, ws = None, st.ws

    def guards_ok(where):
        if big is not None:
            g = torch.cat((big[:guard], big[guard + ws.numel():])).cpu().numpy()
            assert (g == SENT).all(), (where, np.nonzero(g != SENT)[0][:8])

    ref = BR.BeamRef(B, W, V, L, T, eos, 0.0)
    st.init(P)
    ref.init(P)
    guards_ok("init")
    z = np.zeros(B * W, dtype=np.float32)
    for step in range(L):
        pos = P + step - 1
        val, idx = _parent_tables(ref, step, lambda b: _scripted_parents(step, W, b), V, eos)
        infos = ref.update(val, idx, z, z, step, pos)
        if step + 1 < L:  # the script did reorder as intended (at the budget step everything hits)
            assert all(info["parents"] == _scripted_parents(step, W, b) for b, info in enumerate(infos)), step
        _update(st, val, idx, z, z, step, pos, st.x if pos + 1 < T else None)
        full = step % anc_every == anc_every - 1 or step == L - 1
        BR.assert_state_equal(ref, _read(st, ws), step, pos, anc=full, tag=f"T{T}")
        guards_ok(step)
    assert pos + 1 == T or pos + 2 == T
    st.finalize()
    guards_ok("finalize")
    _check_final(st, ref)
    assert (ref.fin_len[:, 0] == L).all()  # no EOS anywhere: every caption finished on the budget step


@pytest.mark.gpu
def test_beam_update_capacity_1024(dev):
    """W * max_len = 1024 (the s_run / s_fin capacity) and T = 1024: 128 steps of scripted reorders (every beam
    from beam W-1, cyclic shifts, permutations, shared parents), state compared each step, ancestry in full every
    16 steps and at the end."""
    _run_reorders(dev, B=2, W=8, V=64, L=128, P=896, T=1024, guard=0, anc_every=16)


@pytest.mark.gpu
def test_beam_update_last_position_and_guards(dev):
    """T = P + max_len - 1, so the last step has pos + 1 == T (no ancestry row of its own to write), on a
    workspace with 64 guard words before and after it that stay untouched after every step and after finalize."""
    _run_reorders(dev, B=3, W=8, V=32, L=16, P=9, T=9 + 16 - 1, guard=64, anc_every=1)


# ---------------------------------------------------------------------------------------------- rowtop + update
def _check_tables(st, logits_f, V, K):
    """The device's row tables against rowtop_ref of the same logits: indices and values exactly, m + ls within
    1e-5 of the fp64 log-sum-exp. Returns the device tables as numpy."""
    R = logits_f.shape[0]
    tv, ti = st.top_val[:R].cpu().numpy(), st.top_idx[:R].cpu().numpy()
    tm, tl = st.top_m[:R].cpu().numpy(), st.top_ls[:R].cpu().numpy()
    val, idx, m, ls = BR.rowtop_ref(logits_f, V, K)
    assert np.array_equal(ti, idx), np.nonzero(ti != idx)
    assert np.array_equal(tv.view(np.int32), val.view(np.int32))
    assert np.abs((tm.astype(np.float64) + tl.astype(np.float64)) - (m + ls)).max() < 1e-5
    return tv, ti, tm, tl


@pytest.mark.gpu
@pytest.mark.parametrize("V,ld,dt,W", [(40, 40, torch.float32, 3), (50257, 50304, torch.bfloat16, 4),
                                       (50257, 50304, torch.bfloat16, 8)])
def test_beam_step_random_tied_logits(dev, V, ld, dt, W):
    """BeamState.step (rowtop, then update) on random logits quantised to 1/4: children of one parent share its
    logits row, so exact ties across beams are the rule. The restatement is fed the device's own row tables, so
    state equality is exact; the tables themselves are checked against rowtop_ref."""
    B, L, P, eos = 2, 6, 4, V - 2
    lp = 0.0 if W == 3 else 1.0
    st, wte, wpe = _state(dev, B, W, V, L, P + L, eos, lp, dt, P + 3)
    ref = BR.BeamRef(B, W, V, L, P + L, eos, lp)
    st.init(P)
    ref.init(P)
    g = torch.Generator().manual_seed(V + W)
    parents = np.tile(np.arange(W), B)
    hit = False
    for step in range(L):
        base = (torch.randn((B * W, ld), generator=g) * 2.0 * 4).round() / 4
        base[:, eos] = base[:, :V].max(dim=1).values - (0.25 * torch.randint(0, 4, (B * W,), generator=g)).float()
        base[:, V:] = float("inf")
        rows = (np.arange(B * W) // W) * W + parents       # row r computes on its parent's history
        logits = base[torch.from_numpy(rows)].to(dt).to(dev)
        pos = P + step - 1
        st.step(logits, step, pos, st.x)
        tv, ti, tm, tl = _check_tables(st, logits.float().cpu().numpy(), V, st.K)
        infos = ref.update(tv, ti, tm, tl, step, pos)
        BR.assert_state_equal(ref, _read(st), step, pos, tag=f"V{V} W{W}")
        exp = ref.next_x(wte, wpe, pos, dt)
        assert torch.equal(st.x.cpu().float(), exp.float()), step
        parents = np.concatenate([info["parents"] for info in infos])
        hit = hit or any(any(info["hits"][:W]) for info in infos)
    # finished scores within 2 ulp of exact on either side (<= 1-ulp powf, one rounded divide): 8 ulp apart cannot swap
    assert hit and not ref.fragile_comparisons(rel=8 * 2.0 ** -23), ref.fragile_comparisons(rel=8 * 2.0 ** -23)[:3]
    _check_final(st, ref)


# ---------------------------------------------------------------------------------------------- rowtop edges
def _bf16_ladder(n):
    """n distinct bf16-exact floats, ascending: consecutive normal bf16 bit patterns round zero."""
    pos = (np.arange(0x0080, 0x7F80, dtype=np.uint32) << np.uint32(16)).view(np.float32)
    allv = np.concatenate((-pos[::-1], pos))
    lo = (allv.size - n) // 2
    return allv[lo: lo + n].copy()


def _edge_rows(V, K, dt):
    """[5, V] fp32 (exact in dt): all equal; two levels with fewer than K on the upper one, so the K-th place falls
    inside the lower tie group, which covers every thread and wave; strictly descending; strictly ascending; three
    levels whose middle tie group sits on every 97th column, so the winners come from different waves, and where one
    thread meets a larger value after two equal ones."""
    x = np.empty((5, V), dtype=np.float32)
    x[0] = 1.5
    x[1] = -2.0
    x[1, [V - 1, V // 2]] = 3.0
    asc = _bf16_ladder(V) if dt == torch.bfloat16 else np.linspace(-4.0, 4.0, V, dtype=np.float32)
    assert (np.diff(asc) > 0).all() or V == 1
    x[2], x[3] = asc[::-1], asc
    x[4] = -1.0
    x[4, ::97] = 0.5
    x[4, V // 3] = 2.0
    if V > 512:  # thread 0 meets two equal values (columns 0, 256), then a larger one: 0 must stay ahead of 256
        x[4, 256], x[4, 512] = 0.5, 2.0
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("K", [8, 16])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_beam_rowtop_edges(dev, dt, K):
    """icap_beam_rowtop for V from 1 to 50257 round the 256-thread stride and round 256 * K, with padding columns
    of +inf / NaN past V that must never appear, tie rows, and the -inf / 0x7fffffff tail for V < K."""
    from icap._lib import call
    from icap.ops import _ld, _stream, dtype_code

    R = 5
    tv = torch.empty((R, K), dtype=torch.float32, device=dev)
    ti = torch.empty((R, K), dtype=torch.int32, device=dev)
    tm = torch.empty(R, dtype=torch.float32, device=dev)
    tl = torch.empty(R, dtype=torch.float32, device=dev)
    for V in (1, 7, 15, 16, 17, 255, 256, 257, 256 * K - 1, 256 * K + 1, 50257):
        ld = V + 9
        x = np.empty((R, ld), dtype=np.float32)
        x[:, :V] = _edge_rows(V, K, dt)
        x[0::2, V:] = np.inf
        x[1::2, V:] = np.nan
        xt = torch.from_numpy(x).to(dt)
        assert torch.equal(xt[:, :V].float(), torch.from_numpy(x[:, :V]))  # the rows are exact in dt
        xd = xt.to(dev)
        tv.fill_(123.0), ti.fill_(-7), tm.fill_(123.0), tl.fill_(123.0)
        call("icap_beam_rowtop", dtype_code(dt), R, V, xd.data_ptr(), _ld(xd), K, tv.data_ptr(), ti.data_ptr(),
             tm.data_ptr(), tl.data_ptr(), _stream())
        val, idx, m, ls = BR.rowtop_ref(x, V, K)
        gi, gv = ti.cpu().numpy(), tv.cpu().numpy()
        assert np.array_equal(gi, idx), (V, gi, idx)
        assert np.array_equal(gv.view(np.int32), val.view(np.int32)), (V, gv, val)
        n = min(V, K)
        assert gi[0, :n].tolist() == list(range(n)), V                   # all equal: ids 0..K-1
        assert (gi[:, :n] < V).all() and np.isfinite(gv[:, :n]).all(), V  # no padding column, no NaN
        assert (gi[:, n:] == BR.PAD_IDX).all() and np.isneginf(gv[:, n:]).all(), V
        got = tm.cpu().numpy().astype(np.float64) + tl.cpu().numpy().astype(np.float64)
        assert np.array_equal(tm.cpu().numpy(), m.astype(np.float32)), V
        assert np.abs(got - (m + ls)).max() < 1e-5, (V, got, m + ls)
