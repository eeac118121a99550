"""Host restatement of the device beam-search state (include/icap.h icap_beam_*), written from that contract and
the oracle's docstring (oracle/icap_oracle.py beam_generate), in numpy with np.float32 arithmetic.

test_beam_refs_cpu.py pins it to the transformers goldens without a GPU; test_beam_kernels_gpu.py and test_beam.py
compare the kernels' workspace with it step by step. It keeps the workspace fields of icap_beam_layout as arrays:
run_score [B, W], run_seq [B, W, L], fin_score / fin_len [B, W], fin_seq [B, W, L], fin_cnt / done [B],
anc [T, R]. Only live fields mean anything: finished slots < fin_cnt, ancestry rows <= pos + 1.

Finished scores: cs / (step + 1) ** lp. With lp == 0 that is cs itself (pow(x, 0) == 1 exactly); otherwise the
restatement keeps the fp64 quotient of the fp32 candidate score (`fin_exact`) and its fp32 rounding, and logs every
comparison between finished scores that a decision rested on (`cmp_log`), so a test can require that no decision
hangs on the last bits of a powf."""

import numpy as np
import torch

NEG = np.float32(-1.0e9)
PAD_IDX = 0x7FFFFFFF
F32 = np.float32


def rowtop_ref(logits, V, K):
    """logits: float array [R, >= V] (the float view of the device row). Returns (val f32 [R, K], idx i32 [R, K],
    m f64 [R], ls f64 [R]): the K largest of the first V columns in a stable descending sort (ties -> lower id;
    past V entries -inf / 0x7fffffff), the row maximum, and log(sum(exp(x - m))) in fp64."""
    x = np.asarray(logits, dtype=np.float32)[:, :V]
    R = x.shape[0]
    val = np.full((R, K), -np.inf, dtype=np.float32)
    idx = np.full((R, K), PAD_IDX, dtype=np.int32)
    order = np.argsort(-x.astype(np.float64), axis=1, kind="stable")[:, :K]
    n = order.shape[1]
    val[:, :n] = np.take_along_axis(x, order, axis=1)
    idx[:, :n] = order
    xd = x.astype(np.float64)
    m = xd.max(axis=1)
    ls = np.log(np.exp(xd - m[:, None]).sum(axis=1))
    return val, idx, m, ls


def ulp32(v):
    """The fp32 unit in the last place at |v| (v a python / fp64 number)."""
    return float(np.spacing(np.abs(np.float32(v))))


class BeamRef:
    def __init__(self, B, W, V, max_len, T, eos, length_penalty, K=None):
        self.B, self.W, self.V, self.L, self.T = B, W, V, max_len, T
        self.eos, self.lp = int(eos), float(length_penalty)
        self.K = K if K is not None else (8 if W <= 4 else 16)
        self.R = B * W
        self.cmp_log = []  # (kind, (num_a, n_a, val_a), (num_b, n_b, val_b)) of finished-score comparisons

    # ------------------------------------------------------------------ state
    def init(self, P):
        B, W, L = self.B, self.W, self.L
        self.run_score = np.full((B, W), NEG, dtype=np.float32)
        self.run_score[:, 0] = 0.0
        self.run_seq = np.full((B, W, L), self.eos, dtype=np.int32)  # not live before step 0
        self.fin_score = np.full((B, W), NEG, dtype=np.float32)
        self.fin_exact = np.full((B, W), float(NEG), dtype=np.float64)
        self.fin_num = np.full((B, W), NEG, dtype=np.float32)  # the fp32 score a finished slot was divided from
        self.fin_n = np.zeros((B, W), dtype=np.int32)           # ... and the step + 1 it was divided by
        self.fin_len = np.zeros((B, W), dtype=np.int32)
        self.fin_seq = np.full((B, W, L), self.eos, dtype=np.int32)
        self.fin_cnt = np.zeros(B, dtype=np.int32)
        self.done = np.zeros(B, dtype=np.int32)
        self.anc = np.full((self.T, self.R), -1, dtype=np.int32)
        self.anc[:P] = np.arange(self.R, dtype=np.int32)[None, :]
        self.run_tok = np.full((B, W), self.eos, dtype=np.int32)
        self.cmp_log = []

    def _norm(self, cs, n):
        """(fp32 value, fp64 value) of cs / n ** lp."""
        if self.lp == 0.0:
            return F32(cs), float(cs)
        q = float(cs) / float(n) ** self.lp
        return F32(q), q

    def update(self, top_val, top_idx, top_m, top_ls, step, pos):
        """One beam step from the row tables (arrays [R, K], [R, K], [R], [R]). Returns one dict per caption with
        what the step decided: cands [(score, beam, tok)], hits, keep (candidate ranks of the next running beams),
        parents, new (ranks recorded as finished), entries [(is_new, rank or kept slot, score)] before the merge,
        merged [(is_new, rank or kept slot)] after it, evicted_kept, done_now, was_done, boundary (score, key of the
        first candidate left out of the 2W)."""
        B, W, V, L, K = self.B, self.W, self.V, self.L, self.K
        tv = np.asarray(top_val, dtype=np.float32).reshape(self.R, K)
        ti = np.asarray(top_idx).reshape(self.R, K)
        tm = np.asarray(top_m, dtype=np.float32).reshape(self.R)
        tl = np.asarray(top_ls, dtype=np.float32).reshape(self.R)
        assert 0 <= step < L and 0 <= pos < self.T
        n = step + 1
        old_anc = self.anc[: pos + 1].copy()
        infos = []
        for b in range(B):
            pool = []
            for i in range(W):
                r = b * W + i
                for k in range(K):
                    x = tv[r, k]
                    if x == -np.inf:  # rows shorter than K end in -inf / 0x7fffffff: no candidates
                        continue
                    sc = F32(F32(F32(x - tm[r]) - tl[r]) + self.run_score[b, i])
                    pool.append((float(sc), i * V + int(ti[r, k]), i, int(ti[r, k]), sc))
            pool.sort(key=lambda c: (-c[0], c[1]))
            assert len(pool) >= 2 * W, "fewer than 2W candidates"
            nxt_same = pool[2 * W][:2] if len(pool) > 2 * W else None
            cands = pool[: 2 * W]
            hits = [tok == self.eos or n == L for _, _, _, tok, _ in cands]
            rsc = [F32(c[4] + (NEG if h else F32(0.0))) for c, h in zip(cands, hits)]
            keep = sorted(range(2 * W), key=lambda j: (-float(rsc[j]), j))[:W]
            old_seq = self.run_seq[b].copy()
            info = dict(cands=[(c[0], c[2], c[3]) for c in cands], hits=hits, keep=keep,
                        parents=[cands[j][2] for j in keep], new=[], entries=[], merged=[], evicted_kept=0,
                        done_now=False,
                        boundary=nxt_same, was_done=bool(self.done[b]))

            def hist(beam, tok):
                h = np.full(L, self.eos, dtype=np.int32)
                h[:step] = old_seq[beam, :step]
                h[step] = tok
                return h

            if not self.done[b]:
                nf = int(self.fin_cnt[b])
                ent = [dict(new=False, src=k, score=self.fin_score[b, k], exact=self.fin_exact[b, k],
                            num=self.fin_num[b, k], n=int(self.fin_n[b, k]), len=int(self.fin_len[b, k]),
                            seq=self.fin_seq[b, k].copy()) for k in range(nf)]
                for j in range(W):
                    if not hits[j]:
                        continue
                    s32, s64 = self._norm(cands[j][4], n)
                    ent.append(dict(new=True, src=j, score=s32, exact=s64, num=cands[j][4], n=n, len=n,
                                    seq=hist(cands[j][2], cands[j][3])))
                    info["new"].append(j)
                # every pair whose order the stable sort decides
                for p in range(len(ent)):
                    for q in range(p + 1, len(ent)):
                        if ent[p]["new"] or ent[q]["new"]:
                            self._log("merge", ent[p], ent[q])
                info["entries"] = [(e["new"], e["src"], float(e["score"])) for e in ent]
                ent = sorted(ent, key=lambda e: -float(e["score"]))  # stable: kept before new, new in rank order
                info["evicted_kept"] = sum(1 for e in ent[W:] if not e["new"])
                ent = ent[:W]
                info["merged"] = [(e["new"], e["src"]) for e in ent]
                for k, e in enumerate(ent):
                    self.fin_score[b, k], self.fin_exact[b, k] = e["score"], e["exact"]
                    self.fin_num[b, k], self.fin_n[b, k] = e["num"], e["n"]
                    self.fin_len[b, k] = e["len"]
                    self.fin_seq[b, k] = e["seq"]
                self.fin_cnt[b] = len(ent)
            for i, j in enumerate(keep):
                self.run_seq[b, i] = hist(cands[j][2], cands[j][3])
                self.run_score[b, i] = rsc[j]
                self.run_tok[b, i] = cands[j][3]
            if not self.done[b] and self.fin_cnt[b] == W:
                best32, best64 = self._norm(self.run_score[b, 0], n)
                worst = dict(score=self.fin_score[b, W - 1], num=self.fin_num[b, W - 1], n=int(self.fin_n[b, W - 1]))
                self._log("done", dict(score=best32, num=self.run_score[b, 0], n=n), worst)
                if not (float(best32) > float(worst["score"])):
                    self.done[b] = 1
                    info["done_now"] = True
            for i, p in enumerate(info["parents"]):
                self.anc[: pos + 1, b * W + i] = old_anc[:, b * W + p]
            infos.append(info)
        if pos + 1 < self.T:
            self.anc[pos + 1] = np.arange(self.R, dtype=np.int32)
        return infos

    def _log(self, kind, a, b):
        self.cmp_log.append((kind, (F32(a["num"]), int(a["n"]), float(a["score"])),
                             (F32(b["num"]), int(b["n"]), float(b["score"]))))

    def fragile_comparisons(self, rel=1e-5):
        """Logged finished-score comparisons that are neither between identical operands (the same fp32 score
        divided at the same step, hence the same bits whatever powf returns) nor separated by >= rel."""
        if self.lp == 0.0:
            return []  # no powf in the value: fp32 scores compare as they are
        bad = []
        for kind, a, b in self.cmp_log:
            if a[0].tobytes() == b[0].tobytes() and a[1] == b[1]:
                continue
            if abs(a[2] - b[2]) >= rel * max(abs(a[2]), abs(b[2])):
                continue
            bad.append((kind, a, b))
        return bad

    def finalize(self):
        """(out int64 [B, L], out_len int32 [B]): slot 0 of the finished list, EOS-padded; a caption without a
        finished hypothesis returns running beam 0 with out_len = L."""
        out = np.full((self.B, self.L), self.eos, dtype=np.int64)
        out_len = np.zeros(self.B, dtype=np.int32)
        for b in range(self.B):
            if self.fin_cnt[b] > 0:
                n, seq = int(self.fin_len[b, 0]), self.fin_seq[b, 0]
            else:
                n, seq = self.L, self.run_seq[b, 0]
            out[b, :n] = seq[:n]
            out_len[b] = n
        return out, out_len

    def next_x(self, wte, wpe, pos, dtype):
        """The next step's input rows [R, D]: wte[token of the new running beam] + wpe[min(pos + 1, n_positions - 1)]
        (wte / wpe CPU tensors of the compute dtype; the sum in fp32, rounded once)."""
        tok = torch.from_numpy(self.run_tok.reshape(-1).astype(np.int64))
        pn = min(pos + 1, wpe.shape[0] - 1)
        return (wte[tok].float() + wpe[pn].float()[None, :]).to(dtype)

    def result(self):
        """ids as beam_decode returns them: finalize() cut to the longest out_len."""
        out, n = self.finalize()
        return out[:, : int(n.max())]


# ---------------------------------------------------------------------- comparing a device workspace with it
def split_workspace(ws, offs, B, W, T, L):
    """ws: int32 numpy array (the workspace read back); offs: ops.beam_layout(). Returns the fields as arrays."""
    R = B * W

    def words(name, n):
        return ws[offs[name]: offs[name] + n]

    return dict(run_score=words("run_score", R).view(np.float32).reshape(B, W),
                run_seq=words("run_seq", R * L).reshape(B, W, L),
                fin_score=words("fin_score", R).view(np.float32).reshape(B, W),
                fin_len=words("fin_len", R).reshape(B, W),
                fin_seq=words("fin_seq", R * L).reshape(B, W, L),
                fin_cnt=words("fin_cnt", B), done=words("done", B),
                anc=words("anc", T * R).reshape(T, R))


def assert_state_equal(ref, dev, step, pos, anc=True, tag=""):
    """Every live field of the device workspace `dev` (split_workspace) against the restatement after `step`.
    Ints and run_score bitwise; fin_score bitwise for lp == 0, else within 4 fp32 ulp of the fp64 quotient
    (one correctly rounded divide + a <= 1-ulp powf, with margin)."""
    where = f"{tag} step {step}"
    assert np.array_equal(dev["run_score"].view(np.int32), ref.run_score.view(np.int32)), \
        (where, dev["run_score"], ref.run_score)
    assert np.array_equal(dev["run_seq"], ref.run_seq), (where, "run_seq")
    assert np.array_equal(dev["fin_cnt"], ref.fin_cnt), (where, dev["fin_cnt"], ref.fin_cnt)
    assert np.array_equal(dev["done"], ref.done), (where, dev["done"], ref.done)
    for b in range(ref.B):
        nf = int(ref.fin_cnt[b])
        assert np.array_equal(dev["fin_len"][b, :nf], ref.fin_len[b, :nf]), (where, b, "fin_len")
        assert np.array_equal(dev["fin_seq"][b, :nf], ref.fin_seq[b, :nf]), (where, b, "fin_seq")
        if ref.lp == 0.0:
            assert np.array_equal(dev["fin_score"][b, :nf].view(np.int32), ref.fin_score[b, :nf].view(np.int32)), \
                (where, b, dev["fin_score"][b, :nf], ref.fin_score[b, :nf])
        else:
            for k in range(nf):
                e = ref.fin_exact[b, k]
                assert abs(float(dev["fin_score"][b, k]) - e) <= 4 * ulp32(e), \
                    (where, b, k, float(dev["fin_score"][b, k]), e)
    if anc:
        n = min(pos + 2, ref.T)
        assert np.array_equal(dev["anc"][:n], ref.anc[:n]), (where, "anc")
