"""The 'stream' and 'parallel_stream' modes of the MemVLA memory bank (PerCogMemBank, reference memvla_arch.py:313-411) on the
GPU against oracle.memvla_oracle.MemBank.

Definition used throughout: ONE oracle MemBank per batch slot (per stream for 'stream'), fed one sample per call with
``training=False`` (a persistent bank; autograd works regardless of the flag) and reset() when the slot's episode changes.

Bounds: the ones tests/test_memvla_gpu.py holds the 'group' batch to — fp32 1e-3 (max-norm relative, helpers.rel_err) for
outputs, bank contents and gradients; bf16 5e-2.  A bias whose true gradient is zero (k_proj: a constant added to every key of
a softmax; the last bias of the timestep embedding: a constant per memory entry) is a sum that cancels to rounding noise, so —
as tests/test_memvla_gpu.py::test_memvla_deferred_gradient_folds_equal_the_per_consumer_writes does — a bias is measured on the
scale of its own gradient or its weight's, whichever is larger.  While a cognition-token bank holds ONE key (steps 0 and 1 of an
episode: N = 1) its softmax is the constant 1, so the true gradient of everything in front of the scores (q / k projections, the
timestep embedder) is exactly zero; autograd returns 0.0 and a kernel that forms dS = P (dP - sum P dP) returns the rounding of
two equal numbers.  Such a gradient is held to one fp32 ulp (2^-23) of the step's largest bank gradient — the floor below.
"""
import os

import numpy as np
import pytest
import torch

from oracle import cogact_oracle as O
from oracle import memvla_oracle as M
from oracle.weights import make_weights

from .helpers import product_config, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {"float32": 1e-3, "bfloat16": 5e-2}
BANK = M.BANK
ROLES = ("cog", "per")                 # the order MemVLAForCausalLM.forward runs them in
B, MEM_LENGTH, STEPS, N_PER = 3, 3, 7, 5          # N_PER: the toy tower has 16 patches (a multiple of 4), so 5
PER_TOKEN, WSEED = 32, 20
SEED = 5                               # chosen on the CPU so that every token merge of the oracle has a clear winner (case 2)
MARGIN = 1e-3
P_DROP = 0.1
# slot -> episode (dataset, file) per step: slot 1 changes episode at step 3, slot 2 at step 5.  At step 3 a slot without history
# sits beside two full banks, at step 5 a full bank, a partly filled one (2 of 3) and one without history share the launches.
EPISODES = [[(0, 0)] * 7, [(0, 1)] * 3 + [(0, 2)] * 4, [(1, 0)] * 5 + [(1, 1)] * 2]


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def weights():
    cfg = O.OracleConfig()
    return cfg, make_weights(M.memvla_shapes(cfg, PER_TOKEN), WSEED)


def build(dtype, train, mode, retrieval_dropout=0.0, mem_length=MEM_LENGTH, consolidate="tome", w=None):
    from dexbotic_amd.model.memvla.memvla_arch import MemVLAConfig, MemVLAForCausalLM
    cfg, w0 = weights()
    w = w or w0
    base = product_config(cfg, dtype)
    mc = MemVLAConfig(llm_config=base.llm_config, mm_vision_tower=base.mm_vision_tower, mm_projector_type="mlp2x_gelu",
                      action_model_type="DiT-T", action_dim=cfg.action_dim, chunk_size=cfg.chunk_size, compute_dtype=dtype,
                      per_token_size=PER_TOKEN, dataloader_type=mode, group_size=3, mem_length=mem_length, retrieval_layers=2,
                      use_timestep_pe=True, fusion_type="gate", consolidate_type=consolidate,
                      retrieval_dropout=retrieval_dropout)
    m = MemVLAForCausalLM(mc, device=DEV, train=train)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    m.train(train)
    if train:
        m.store.set_expected([n for n in m.store.slots if not n.startswith(BANK)])
    return cfg, m


def dims(cfg):
    return {"cog": (1, cfg.hidden_size), "per": (N_PER, PER_TOKEN)}


def frames(episodes):
    """timestep of every (slot, step): the frame's index inside its episode"""
    out = []
    for eps in episodes:
        row, k = [], 0
        for s, e in enumerate(eps):
            k = k + 1 if s > 0 and e == eps[s - 1] else 0
            row.append(float(k))
        out.append(row)
    return out


def make_inputs(cfg, seed, nslots, steps):
    rs = np.random.RandomState(seed)
    tok = {r: rs.standard_normal((steps, nslots) + dims(cfg)[r]).astype(np.float32) for r in ROLES}
    proj = {r: rs.standard_normal((steps, nslots) + dims(cfg)[r]).astype(np.float32) for r in ROLES}
    return tok, proj


class OracleMasks:
    """the dropout masks the oracle consumes, in its own order (per slot: per layer: attention, FFN hidden, FFN output), kept
    under (step, role, slot, layer, kind) so that the batched masks can be assembled from them"""

    def __init__(self, seed, p):
        self.rs, self.p, self.taken, self.ctx, self.k = np.random.RandomState(seed), p, {}, None, 0

    def at(self, step, role, slot):
        self.ctx, self.k = (step, role, slot), 0

    def __call__(self, shape):
        m = (self.rs.random_sample(shape) >= self.p).astype(np.float32) / (1.0 - self.p)
        self.taken[self.ctx + (self.k // 3, self.k % 3)] = m
        self.k += 1
        return torch.from_numpy(m)


class watch_margins:
    """the oracle's own consolidation with its similarities looked at first: ``.smallest`` = the least gap between the largest and
    the second-largest similarity over all token merges run inside the block"""

    def __enter__(self):
        self.smallest = np.inf
        self.orig = orig = M.MemBank._consolidate
        this = self

        def cons(bank_self, role, eid, feat, timestep):
            bank = bank_self.banks[role].get(eid, [])
            if len(bank) + 1 > bank_self.mem_length:
                fs = [f for _, f in bank] + [feat.detach()]
                cos = torch.nn.functional.cosine_similarity
                sims = sorted(float(cos(a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1]), dim=1).mean())
                              for a, b in zip(fs[:-1], fs[1:]))
                this.smallest = min(this.smallest, sims[-1] - sims[-2])
            return orig(bank_self, role, eid, feat, timestep)
        M.MemBank._consolidate = cons
        return self

    def __exit__(self, *exc):
        M.MemBank._consolidate = self.orig
        return False


def oracle_slots(seed=SEED, episodes=EPISODES, steps=STEPS, grads=True, masks=None, monkeypatch=None, clear=True):
    """every slot through its own oracle bank.  ``clear=False``: evaluation — the reference then keys slot i as (i, 0, 0) whatever
    the episode ids say (memvla_arch.py:345-346), so nothing is cleared and the seven frames of a slot are ONE episode.  Returns outs[role][step] ([B, N, D]), per-step gradients (one backward per step of
    sum(out * proj) over both roles), the final banks per slot and the smallest arg-max margin of all token merges."""
    cfg, w = weights()
    sd = {k: torch.from_numpy(v).clone() for k, v in w.items()}
    names = [k for k in sd if k.startswith(BANK)]
    for k in names:
        sd[k].requires_grad_(grads)
    tok, proj = make_inputs(cfg, seed, len(episodes), steps)
    ts = frames(episodes)
    banks = [M.MemBank(MEM_LENGTH) for _ in episodes]
    if masks is not None:
        orig_block = M.cross_block
        monkeypatch.setattr(M, "cross_block", lambda *a, **kw: orig_block(*a, **dict(kw, mask_fn=masks)))
    with watch_margins() as watch:
        outs = {r: [] for r in ROLES}
        gsteps = []
        for s in range(steps):
            x = {r: torch.from_numpy(tok[r][s]).clone().requires_grad_(grads) for r in ROLES}
            loss = 0.0
            for b, eps in enumerate(episodes):
                if clear and s > 0 and eps[s] != eps[s - 1]:
                    banks[b].reset()
            for r in ROLES:
                rows = []
                for b in range(len(episodes)):
                    if masks is not None:
                        masks.at(s, r, b)
                    rows.append(banks[b].process(sd, r, x[r][b:b + 1], [(0, 0)], [torch.tensor(ts[b][s])], training=False))
                out = torch.cat(rows, 0)
                outs[r].append(out.detach().numpy())
                loss = loss + (out * torch.from_numpy(proj[r][s])).sum()
            if grads:
                for k in names:
                    sd[k].grad = None
                loss.backward()
                g = {k: sd[k].grad.numpy().copy() for k in names if sd[k].grad is not None}
                g.update({"tokens/" + r: x[r].grad.numpy().copy() for r in ROLES})
                gsteps.append(g)
    final = [{r: [(float(t), f.numpy()) for t, f in bk.banks[r].get((0, 0), [])] for r in ROLES} for bk in banks]
    return dict(outs=outs, grads=gsteps, final=final, margin=watch.smallest, tok=tok, proj=proj, ts=ts)


_CACHE = {}


def oracle_reference(train=True):
    if train not in _CACHE:
        _CACHE[train] = oracle_slots(clear=train, grads=train)
    return _CACHE[train]


def product_slots(m, ref, dtype, train, grads=False, episodes=EPISODES, steps=STEPS, before_role=None):
    tdt = getattr(torch, dtype)
    bank = m.model.per_cog_mem_bank
    st = m.store
    outs, gsteps = {r: [] for r in ROLES}, []
    for s in range(steps):
        if train:
            st.begin_step()
        eids = [eps[s] for eps in episodes]
        ts = T(np.array([row[s] for row in ref["ts"]], dtype=np.float32))
        x = {r: T(ref["tok"][r][s], tdt).requires_grad_(grads) for r in ROLES}
        loss = 0.0
        with torch.set_grad_enabled(train):
            for r in ROLES:
                if before_role is not None:
                    before_role(s, r)
                out = (bank.process_batch_cog if r == "cog" else bank.process_batch_per)(x[r], eids, ts)
                assert out.shape == x[r].shape
                outs[r].append(out.detach().float().cpu().numpy())
                if grads:
                    loss = loss + (out * T(ref["proj"][r][s], tdt)).sum()
        if grads:
            loss.backward()
            st.flush_wgrads()
            torch.cuda.synchronize()
            g = {n: st.g(n).float().cpu().numpy().copy() for n in st.slots if n.startswith(BANK)}
            g.update({"tokens/" + r: x[r].grad.float().cpu().numpy() for r in ROLES})
            gsteps.append(g)
    return outs, gsteps


def check_outputs(outs, ref, tol, what):
    worst = 0.0
    for r in ROLES:
        for s, (a, b) in enumerate(zip(outs[r], ref["outs"][r])):
            assert np.isfinite(a).all(), (what, r, s)
            for slot in range(a.shape[0]):
                worst = max(worst, rel_err(a[slot], b[slot]))
    print(f"{what}: worst output distance {worst:.2e} (bound {tol:.0e})")
    assert worst < tol, (what, worst)


def check_banks(bank, ref, keys, tol, what):
    worst = 0.0
    for slot, key in enumerate(keys):
        for r in ROLES:
            got, want = bank.entries(r, key), ref["final"][slot][r]
            assert len(got) == len(want) and len(want) <= MEM_LENGTH, (what, slot, r, len(got), len(want))
            for (t, f), (tw, fw) in zip(got, want):
                assert abs(float(t) - tw) <= 1e-6 * max(1.0, abs(tw)), (what, slot, r, float(t), tw)
                worst = max(worst, rel_err(f.float().cpu().numpy(), fw))
    print(f"{what}: worst bank-entry distance {worst:.2e} (bound {tol:.0e})")
    assert worst < tol, (what, worst)


# ------------------------------------------------------------------------------------------------------------- cases 1, 2, 3
def test_oracle_token_merges_have_a_clear_winner():
    """case 2: the token merge takes an arg-max that rounding may flip, so the comparison below is only meaningful when the
    oracle's largest and second-largest similarity are more than 1e-3 apart at EVERY consolidation of the schedule"""
    for train in (True, False):
        ref = oracle_reference(train)
        assert all(len(ref["final"][0][r]) == MEM_LENGTH for r in ROLES)          # slot 0 overflowed and merged
        print(f"smallest arg-max margin over all consolidations ({'train' if train else 'eval'}): {ref['margin']:.3e}")
        assert np.isfinite(ref["margin"]) and ref["margin"] > MARGIN, ref["margin"]


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_parallel_stream_forward_matches_the_per_slot_oracle(dtype, train):
    """case 1: 7 steps of 3 slots, mem_length 3: every step's output and, after the last step, every bank.  Training: slot 1
    changes episode at step 3 and slot 2 at step 5 (their banks are cleared).  Evaluation: the same frames, never cleared."""
    ref = oracle_reference(train)
    assert ref["margin"] > MARGIN
    cfg, m = build(dtype, train, "parallel_stream")
    outs, _ = product_slots(m, ref, dtype, train)
    check_outputs(outs, ref, TOL[dtype], f"parallel_stream {dtype} {'train' if train else 'eval'}")
    keys = [(b,) + EPISODES[b][-1] for b in range(B)] if train else [(b, 0, 0) for b in range(B)]
    bank = m.model.per_cog_mem_bank
    check_banks(bank, ref, keys, TOL[dtype], f"parallel_stream {dtype} banks")
    if train:                                       # the banks of the episodes the slots left were cleared
        assert bank.entries("per", (1,) + EPISODES[1][0]) == [] and bank.entries("cog", (2,) + EPISODES[2][0]) == []
    with pytest.raises(ValueError):                 # sized by the first batch
        bank.process_batch_cog(torch.zeros(B + 1, 1, cfg.hidden_size, device=DEV, dtype=getattr(torch, dtype)),
                               [(0, 0)] * (B + 1), torch.zeros(B + 1, device=DEV))
    bank.reset()
    assert bank.entries("per", keys[0]) == [] and not bank.slot_banks["per"]


def test_parallel_stream_gradients_match_the_oracle_autograd():
    """case 3: one backward per step of a fixed random projection of that step's outputs (banks detached): the gradients of the
    retrieval blocks, the gate fusion, the timestep embedders and the input tokens, every step.  Steps 3 and 5 hold a slot
    without history (its tokens are reached through keys and values) beside slots with history."""
    ref = oracle_reference()
    cfg, m = build("float32", True, "parallel_stream")
    outs, gsteps = product_slots(m, ref, "float32", True, grads=True)
    check_outputs(outs, ref, TOL["float32"], "parallel_stream fp32 train + backward")
    worst, worst_key = 0.0, None
    for s, (g, gw) in enumerate(zip(gsteps, ref["grads"])):
        assert set(k for k in gw if not k.startswith("tokens/")) == set(k for k in g if not k.startswith("tokens/"))
        floor = 2.0 ** -23 * max(float(np.abs(v).max()) for k, v in gw.items() if not k.startswith("tokens/")) / TOL["float32"]
        for k, want in gw.items():
            if k.startswith("tokens/"):
                for slot in range(B):              # every slot's token gradient on its own scale
                    d = rel_err(g[k][slot], want[slot])
                    if d > worst:
                        worst, worst_key = d, (s, k, slot)
                continue
            scale = float(np.abs(want).max())
            if k.endswith(".bias") and k[:-4] + "weight" in gw:
                scale = max(scale, float(np.abs(gw[k[:-4] + "weight"]).max()))
            d = float(np.abs(g[k].reshape(want.shape) - want).max()) / max(scale, floor)
            if d > worst:
                worst, worst_key = d, (s, k)
    print(f"worst gradient distance over {len(gsteps)} steps: {worst:.2e} at {worst_key} (bound 1e-3)")
    assert worst < TOL["float32"], (worst, worst_key)
    # the slots without history at steps 3 and 5 did receive a gradient through their own keys / values
    assert np.abs(ref["grads"][3]["tokens/per"][1]).max() > 0 and np.abs(gsteps[3]["tokens/per"][1]).max() > 0


# --------------------------------------------------------------------------------------------------------------------- case 4
def test_parallel_stream_retrieval_dropout_with_injected_masks(monkeypatch):
    """case 4: retrieval dropout 0.1 while training.  The oracle draws per slot; the product asks set_mask_fn ONCE per role and
    layer for the batched shapes (B, H, N, cap N), (B N, 4 D), (B N, D): the batched mask is assembled from the per-slot masks
    the oracle consumed.  Columns behind a slot's keys are never read — they are filled with NaN here to prove it."""
    masks = OracleMasks(79, P_DROP)
    ref = oracle_slots(grads=False, masks=masks, monkeypatch=monkeypatch)
    assert ref["margin"] > MARGIN, ref["margin"]                 # (case 2, for this run's merges)
    cfg, m = build("float32", True, "parallel_stream", retrieval_dropout=P_DROP)
    bank = m.model.per_cog_mem_bank
    state = {"ctx": None, "k": 0, "calls": 0}

    def before_role(s, r):
        state["ctx"], state["k"] = (s, r), 0

    def feed(shape):
        s, r = state["ctx"]
        layer, kind = state["k"] // 3, state["k"] % 3
        state["k"] += 1
        state["calls"] += 1
        N, D = dims(cfg)[r]
        if kind == 0:
            assert shape == (B, 4, N, (MEM_LENGTH + 1) * N), shape
            out = np.full(shape, np.nan, dtype=np.float32)
            for b in range(B):
                mk = masks.taken[(s, r, b, layer, 0)]
                out[b, :, :, :mk.shape[-1]] = mk[0]
            return out
        assert shape == (B * N, 4 * D if kind == 1 else D), shape
        return np.concatenate([masks.taken[(s, r, b, layer, kind)].reshape(N, -1) for b in range(B)], 0)
    bank.set_mask_fn(feed)
    outs, _ = product_slots(m, ref, "float32", True, before_role=before_role)
    assert state["calls"] == STEPS * len(ROLES) * 2 * 3
    check_outputs(outs, ref, TOL["float32"], "parallel_stream fp32 train, dropout 0.1")
    check_banks(bank, ref, [(b,) + EPISODES[b][-1] for b in range(B)], TOL["float32"], "dropout banks")


# --------------------------------------------------------------------------------------------------------------------- case 5
STREAM_SEED = 4
STREAM = [[("A", (3, 0)), ("A", (3, 0)), ("B", (3, 1)), ("B", (3, 1))], [("B", (3, 1)), ("B", (3, 1)), ("C", (4, 0)), ("C", (4, 0))]]


def oracle_stream(train):
    """one bank, cleared at each change of episode while training; evaluation is one episode (0, 0) that is never cleared"""
    cfg, w = weights()
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    tok, _ = make_inputs(cfg, STREAM_SEED, 4, len(STREAM))
    outs, prev, k = {r: [] for r in ROLES}, None, -1
    ts = []
    for s, batch in enumerate(STREAM):
        row = []
        for name, _ in batch:
            k = k + 1 if name == prev else 0
            prev = name
            row.append(float(k))
        ts.append(row)
    banks = {r: M.MemBank(MEM_LENGTH) for r in ROLES}          # the roles run one after the other over the batch
    with torch.no_grad(), watch_margins() as watch:
        for r in ROLES:
            prev = None
            for s, batch in enumerate(STREAM):
                rows = []
                for i, (name, _) in enumerate(batch):
                    if train and prev is not None and name != prev:
                        banks[r].reset()
                    prev = name
                    rows.append(banks[r].process(sd, r, torch.from_numpy(tok[r][s][i:i + 1]), [(0, 0)], [torch.tensor(ts[s][i])],
                                                 training=False))
                outs[r].append(torch.cat(rows, 0).numpy())
    final = [{r: [(float(t), f.numpy()) for t, f in banks[r].banks[r].get((0, 0), [])] for r in ROLES}]
    return dict(outs=outs, final=final, tok=tok, ts=ts, margin=watch.smallest)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_stream_mode_clears_the_bank_at_each_change_of_episode(train):
    """case 5: batches A A B B and B B C C.  Training: the bank is cleared at A -> B inside the first batch and at B -> C inside the
    second, and episode B carries over from one batch to the next.  Evaluation: every sample is episode (0, 0)."""
    ref = oracle_stream(train)
    print(f"smallest arg-max margin of the stream's token merges: {ref['margin']:.3e}")
    assert np.isfinite(ref["margin"]) and ref["margin"] > MARGIN, ref["margin"]       # (case 2, for this schedule)
    cfg, m = build("float32", train, "stream")
    bank = m.model.per_cog_mem_bank
    outs = {r: [] for r in ROLES}
    for s, batch in enumerate(STREAM):
        if train:
            m.store.begin_step()
        eids = [e for _, e in batch]
        ts = T(np.array(ref["ts"][s], dtype=np.float32))
        with torch.set_grad_enabled(train):
            for r in ROLES:
                x = T(ref["tok"][r][s])
                out = (bank.process_batch_cog if r == "cog" else bank.process_batch_per)(x, eids, ts)
                outs[r].append(out.detach().cpu().numpy())
    check_outputs(outs, ref, TOL["float32"], f"stream {'train' if train else 'eval'}")
    check_banks(bank, ref, [STREAM[1][-1][1] if train else (0, 0)], TOL["float32"], "stream banks")
    if train:
        assert bank.entries("per", (3, 0)) == [] and bank.entries("cog", (3, 1)) == []
        assert len(bank.entries("per", (4, 0))) == 2


# --------------------------------------------------------------------------------------------------------------------- case 6
def test_inference_action_is_bit_identical_across_dataloader_modes(golden_dir):
    """case 6: a served episode is slot 0; a 'parallel_stream' (and a 'stream') model answers exactly as a 'group' model"""
    g = np.load(os.path.join(golden_dir, "memvla_t1.npz"), allow_pickle=False)
    nf = min(4, g["infer_frames"].shape[0])
    runs = {}
    for mode in ("group", "parallel_stream", "stream"):
        cfg, m = build("float32", False, mode)
        norms = {"min": [-1.0] * cfg.action_dim, "max": [1.0] * cfg.action_dim}
        runs[mode] = np.stack([np.array(m.inference_action(
            T(g["infer_prompt"]), T(g["infer_frames"][f:f + 1]), "True" if f == 0 else "False",
            {"cfg_scale": 1.5, "num_ddim_steps": 10, "action_norms": norms, "use_graph": False}, noise=T(g["infer_inits"][f])))
            for f in range(nf)])
        assert len(m.model.per_cog_mem_bank.entries("per", (0, 0, 0) if mode == "parallel_stream" else (0, 0))) == min(nf, MEM_LENGTH)
    assert nf == 4 and np.isfinite(runs["group"]).all()
    assert np.array_equal(runs["parallel_stream"], runs["group"])
    assert np.array_equal(runs["stream"], runs["group"])


# --------------------------------------------------------------------------------------------------------------------- case 7
SHAPES = [(3, 5, 72), (1, 5, 72), (4, 1, 72), (2, 3, 256)]          # (B, N, D): D = 72 is no multiple of 64; one slot; one token


def _rand_bank(Bn, cap, N, D, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    feat = torch.randn((Bn, cap, N, D), generator=gen).to(DEV, dtype)
    ts = (torch.rand((Bn, cap), generator=gen) * 50).to(DEV)
    return feat, ts


def _count_patterns(Bn, cap):
    ml = cap - 1
    return {"zero": [0] * Bn, "full": [ml] * Bn, "mixed": [(0, ml, 1, 2)[b % 4] for b in range(Bn)]}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stage_append_and_stage_bwd_kernels(shape, dtype):
    from dexbotic_amd import kernels as K
    Bn, N, D = shape
    cap = 4
    for name, cnt in _count_patterns(Bn, cap).items():
        feat, ts = _rand_bank(Bn, cap, N, D, dtype, 1)
        gen = torch.Generator().manual_seed(2)
        tokens = torch.randn((Bn, N, D), generator=gen).to(DEV, dtype)
        steps = (torch.rand(Bn, generator=gen) * 9).to(DEV)
        counts = torch.tensor(cnt, dtype=torch.int32, device=DEV)
        mem, ts_eff, kv_len = K.bank_stage_fwd(feat, ts, counts, tokens, steps)
        want_mem, want_ts = torch.zeros_like(feat), torch.zeros_like(ts)
        for b, n in enumerate(cnt):
            if n > 0:
                want_mem[b, :n], want_ts[b, :n] = feat[b, :n], ts[b, :n]
            else:
                want_mem[b, 0], want_ts[b, 0] = tokens[b], steps[b]
        assert torch.equal(mem, want_mem) and torch.equal(ts_eff, want_ts), name
        assert kv_len.tolist() == [max(n, 1) * N for n in cnt], name
        for b, n in enumerate(cnt):                 # zeros (not merely finite) behind kv_len
            assert not mem[b].reshape(cap * N, D)[max(n, 1) * N:].any(), (name, b)
        dmem = torch.randn((Bn, cap, N, D), generator=gen).to(DEV, dtype)
        dtok = K.bank_stage_bwd(dmem, counts)
        want = torch.stack([dmem[b, 0] if n == 0 else torch.zeros_like(dmem[b, 0]) for b, n in enumerate(cnt)])
        assert torch.equal(dtok, want), name
        f2, t2 = feat.clone(), ts.clone()
        K.bank_append(f2, t2, counts, tokens, steps)
        wf, wt = feat.clone(), ts.clone()
        for b, n in enumerate(cnt):
            wf[b, n], wt[b, n] = tokens[b], steps[b]
        assert torch.equal(f2, wf) and torch.equal(t2, wt), name
    # a count outside [0, cap] is clamped: nothing outside the buffers is read or written
    feat, ts = _rand_bank(Bn, cap, N, D, dtype, 3)
    f2, t2 = feat.clone(), ts.clone()
    wild = torch.tensor([(-5, 1000)[b % 2] for b in range(Bn)], dtype=torch.int32, device=DEV)
    K.bank_append(f2, t2, wild, tokens, steps)
    for b in range(Bn):
        if b % 2:                                   # 1000 -> cap: a full slot is left alone
            assert torch.equal(f2[b], feat[b]) and torch.equal(t2[b], ts[b])
        else:                                       # -5 -> 0
            assert torch.equal(f2[b, 0], tokens[b]) and torch.equal(f2[b, 1:], feat[b, 1:])
    mem, ts_eff, kv_len = K.bank_stage_fwd(feat, ts, wild, tokens, steps)
    assert kv_len.tolist() == [(N, cap * N)[b % 2] for b in range(Bn)]


@pytest.mark.parametrize("fifo", [False, True], ids=["tome", "fifo"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batched_consolidate_is_bit_equal_to_one_call_per_slot(shape, dtype, fifo):
    """counts + 1 > mem_length -> the slot is consolidated exactly as dxa_bank_consolidate does it alone; the others are untouched.
    Slot 0 carries a planted tie (entries 0 = 1 = 2: pairs 0 and 1 both have similarity 1, the first wins); the last slot has a
    zero token in entry 1 (the eps path of the norms)."""
    from dexbotic_amd import kernels as K
    Bn, N, D = shape
    cap = 5
    ml = cap - 1
    for name, cnt in {"full": [ml] * Bn, "none": [ml - 1] * Bn, "mixed": [(ml, 1, ml, 0)[b % 4] for b in range(Bn)]}.items():
        feat, ts = _rand_bank(Bn, cap, N, D, dtype, 4)
        feat[0, 1] = feat[0, 0]
        feat[0, 2] = feat[0, 0]
        feat[Bn - 1, 1, N - 1] = 0
        counts = torch.tensor(cnt, dtype=torch.int32, device=DEV)
        want_f, want_t, ts0 = feat.clone(), ts.clone(), ts.clone()
        for b, n in enumerate(cnt):
            if n + 1 > ml:
                fb, tb = want_f[b].clone(), want_t[b].clone()
                K.bank_consolidate(fb, tb, n + 1, torch.empty(cap, device=DEV), fifo=fifo)
                want_f[b], want_t[b] = fb, tb
        sims = torch.empty(Bn * (cap - 1), device=DEV)
        K.bank_consolidate_batched(feat, ts, counts, 1, ml, None if fifo else sims, fifo=fifo)
        # the entry behind a consolidated bank (index n) is dead storage in both; everything else must agree bit for bit
        for b, n in enumerate(cnt):
            live = n if n + 1 > ml else cap
            assert torch.equal(feat[b, :live], want_f[b, :live]) and torch.equal(ts[b, :live], want_t[b, :live]), (name, b)
        if name == "full" and not fifo:             # the tie: pair 0 was merged, so entry 1 now holds what entry 2 held
            assert torch.equal(ts[0, 0], 0.5 * (ts0[0, 0] + ts0[0, 1])) and torch.equal(ts[0, 1], ts0[0, 2])
