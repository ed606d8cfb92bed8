"""tests/golden/qwen3_t1.npz is what the installed transformers.Qwen3Model computes: scripts/gen_golden_qwen3.py is re-run on the CPU
and compared with the committed archive (inputs and weights bit for bit, results within fp32 rounding of a re-run), so a drift of
the library or an edited fixture shows."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_regenerates_from_the_installed_library(golden_dir):
    spec = importlib.util.spec_from_file_location("_gen_golden_qwen3", os.path.join(ROOT, "scripts", "gen_golden_qwen3.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    new = gen.compute()
    old = np.load(os.path.join(golden_dir, "qwen3_t1.npz"), allow_pickle=False)
    assert sorted(old.files) == sorted(new)
    exact = {"seed", "cfg", "rope_theta", "rms_norm_eps", "names", "inputs_embeds", "loss_weight"}
    for k in old.files:
        a, b = old[k], np.asarray(new[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if k in exact or k.startswith("w/"):
            assert np.array_equal(a, b), k
        else:
            # the same fp32 program on another host / thread count: summation order only
            assert np.allclose(a, b, rtol=1e-4, atol=1e-5 * max(1.0, float(np.abs(a).max()))), (k, float(np.abs(a - b).max()))
    # the properties the fixture is there for
    V, H, I, NL, NH, NKV, D = (int(v) for v in old["cfg"])
    assert NH * D != H and old["w/layers.0.self_attn.q_proj.weight"].shape == (NH * D, H)
    assert not any(str(n).endswith("bias") for n in old["names"])
    for n in ("q_norm", "k_norm"):
        w = old[f"w/layers.0.self_attn.{n}.weight"]
        assert w.shape == (D,) and float(np.abs(w - 1).max()) > 0.3
    full = np.concatenate([old["cached_prefill"], old["cached_steps"]], axis=1)
    assert np.allclose(full, old["last_hidden_state"], atol=1e-5)
    assert os.path.getsize(os.path.join(golden_dir, "qwen3_t1.npz")) < (1 << 20)
