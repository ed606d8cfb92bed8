"""tests/golden/qwen3_d64.npz is what the installed transformers.Qwen3Model computes: scripts/gen_golden_qwen3_decode.py is re-run on
the CPU and compared with the committed archive (inputs and weights bit for bit, fp32 results within fp32 rounding of a re-run, the
bf16 walk within bf16 rounding), so a drift of the library or an edited fixture shows."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_regenerates_from_the_installed_library(golden_dir):
    spec = importlib.util.spec_from_file_location("_gen_golden_qwen3_decode", os.path.join(ROOT, "scripts", "gen_golden_qwen3_decode.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    new = gen.compute()
    path = os.path.join(golden_dir, "qwen3_d64.npz")
    old = np.load(path, allow_pickle=False)
    assert sorted(old.files) == sorted(new)
    exact = {"seed", "cfg", "rope_theta", "rms_norm_eps", "names", "inputs_embeds"}
    for k in old.files:
        a, b = old[k], np.asarray(new[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if k in exact or k.startswith("w/"):
            assert np.array_equal(a, b), k
        elif k == "cached_steps_bf16":
            # the same bf16 program on another host / thread count: a changed summation order flips roundings of 2^-8 that the two
            # layers carry on, so a re-run is held to a few bf16 steps of the largest value, not to fp32 rounding
            assert float(np.abs(a - b).max()) <= 4 * 2.0 ** -8 * float(np.abs(a).max()), (k, float(np.abs(a - b).max()))
        else:
            # the same fp32 program on another host / thread count: summation order only
            assert np.allclose(a, b, rtol=1e-4, atol=1e-5 * max(1.0, float(np.abs(a).max()))), (k, float(np.abs(a - b).max()))
    # the properties the fixture is there for
    V, H, I, NL, NH, NKV, D = (int(v) for v in old["cfg"])
    assert D == 64 and NH * D != H and NH % NKV == 0 and NH // NKV == 2
    assert old["w/layers.0.self_attn.q_proj.weight"].shape == (NH * D, H)
    assert not any(str(n).endswith("bias") for n in old["names"])
    assert not any(k.startswith("grad") for k in old.files)
    for n in ("q_norm", "k_norm"):
        w = old[f"w/layers.0.self_attn.{n}.weight"]
        assert w.shape == (D,) and float(np.abs(w - 1).max()) > 0.3
    assert old["inputs_embeds"].shape == (1, 17, H) and old["cached_prefill"].shape == (1, 11, H)
    assert old["cached_steps"].shape == old["cached_steps_bf16"].shape == (1, 6, H)
    full = np.concatenate([old["cached_prefill"], old["cached_steps"]], axis=1)
    assert np.allclose(full, old["last_hidden_state"], atol=1e-5)
    # HF's own bf16 walk stays within bf16 reach of its fp32 walk on every step: the yardstick of the GPU test is a sane one
    for t in range(6):
        gap = gen.rel(old["cached_steps_bf16"][:, t], old["cached_steps"][:, t])
        assert 1e-3 < gap < 3e-2, (t, gap)
    assert os.path.getsize(path) < (1 << 20)
