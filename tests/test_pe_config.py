"""The Perception Encoder tower without a GPU: the registered configuration against the reference's values (written out here), the
state-dict keys and shapes of the native tower against the list the reference's class produced (tests/golden/pe_t1.npz), the token
count after the two stride-2 convolutions, the factory's dispatch, the refusals, the weight recipe against the stored checksums,
and the new entry points in the header and the ctypes table."""
import os
import re

import numpy as np
import pytest
import torch

from . import muvla_weights as MW
from . import pe_weights as PW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = "model.mm_vision_tower.vision_tower."
NEW_SYMBOLS = ("dxa_rope2d_fwd", "dxa_rope2d_bwd", "dxa_layerscale_residual_fwd", "dxa_layerscale_residual_bwd",
               "dxa_layerscale_bwd_rows", "dxa_conv3x3s2_im2col", "dxa_conv3x3s2_col2im")
_G = {}


def load(golden_dir):
    if not _G:
        _G["g"] = np.load(os.path.join(golden_dir, "pe_t1.npz"), allow_pickle=False)
    return _G["g"]


def tiny_config(g, **over):
    from dexbotic_amd.model import PerceptionEncoderConfig
    patch, width, layers, heads, ratio, image, _ = (int(v) for v in g["cfg"])
    kw = dict(patch_size=patch, width=width, layers=layers, heads=heads, mlp_ratio=float(ratio), output_dim=None,
              ls_init_value=float(g["ls_init"]), image_size=image, use_cls_token=True, pool_type="none", use_ln_pre=True,
              use_ln_post=False)
    kw.update(over)
    return PerceptionEncoderConfig(**kw)


def cpu_tower(cfg):
    from dexbotic_amd.engine import ParamStore, attach_parameters
    from dexbotic_amd.model.modules.mm_vision.builder import build_vision_tower
    st = ParamStore("cpu", torch.float32)
    tower = build_vision_tower(cfg, st)
    st.finalize(train=False)
    attach_parameters(tower, st)
    return st, tower


def test_registered_config_equals_the_references():
    """pe_configuration.py:57-69 (PE_LANG_L14_728) over the base defaults :16-31"""
    from dexbotic_amd.model.modules.mm_vision.pe import get_config
    c = get_config("pe_lang_l14_728")
    want = dict(patch_size=14, width=1024, layers=23, heads=16, mlp_ratio=4.0, output_dim=None, ls_init_value=0.1, drop_path=0.0,
                image_size=728, use_abs_posemb=True, use_cls_token=True, use_rope2d=True, pool_type="none", attn_pooler_heads=8,
                use_ln_pre=True, use_ln_post=False, layer_types=[], sliding_window_size=-1)
    have = c.to_dict()
    assert have.pop("model_type") == "perception_encoder"
    assert have == want
    with pytest.raises(ValueError, match="Unknown configuration name"):
        get_config("pe_lang_l14")


def test_base_config_defaults_and_from_any():
    from dexbotic_amd.model import PerceptionEncoderConfig
    c = PerceptionEncoderConfig(patch_size=4, width=64, layers=2, heads=2, mlp_ratio=2.0, output_dim=None)
    assert (c.ls_init_value, c.image_size, c.use_cls_token, c.pool_type, c.use_ln_pre, c.use_ln_post) == (None, 224, False, "attn", True, True)
    d = c.to_dict()
    d["unknown_key"] = 1
    assert PerceptionEncoderConfig.from_any(d) == c
    assert PerceptionEncoderConfig.from_any(c) is c
    assert PerceptionEncoderConfig.from_any("pe_lang_l14_728").width == 1024

    class Obj:
        pass
    o = Obj()
    o.__dict__.update(c.to_dict())
    assert PerceptionEncoderConfig.from_any(o) == c


def test_state_dict_keys_and_shapes_equal_the_references(golden_dir):
    g = load(golden_dir)
    st, tower = cpu_tower(tiny_config(g))
    want = {PREFIX + str(k): s for k, s in zip(g["w_keys"], MW.unpack_shapes(g["w_shapes"]))}
    have = {k: tuple(v.shape) for k, v in tower.state_dict().items()}
    assert have == want
    assert set(st.slots) == set(want)
    assert want[PREFIX + "transformer.resblocks.1.attn.in_proj_weight"] == (192, 64)
    assert want[PREFIX + "vit_downsampler2.weight"] == (256, 128, 3, 3)
    assert tower.unused_parameter_names() == []
    # the interface of the other towers; hidden_size is the width although the output rows are four times as wide
    assert (tower.hidden_size, tower.num_patches, tower.dtype, str(tower.device)) == (64, 4, torch.float32, "cpu")
    assert tower.config is tower.cfg and tuple(tower.dummy_feature.shape) == (1, 256)


def test_flags_change_the_registered_tensors(golden_dir):
    g = load(golden_dir)
    base = set(cpu_tower(tiny_config(g))[0].slots)
    no_cls = cpu_tower(tiny_config(g, use_cls_token=False))[0]
    assert base - set(no_cls.slots) == {PREFIX + "class_embedding"} and no_cls.slots[PREFIX + "positional_embedding"].shape == (36, 64)
    assert set(cpu_tower(tiny_config(g, use_ln_post=True))[0].slots) - base == {PREFIX + "ln_post.weight", PREFIX + "ln_post.bias"}
    assert base - set(cpu_tower(tiny_config(g, use_ln_pre=False))[0].slots) == {PREFIX + "ln_pre.weight", PREFIX + "ln_pre.bias"}
    no_ls = set(cpu_tower(tiny_config(g, ls_init_value=None))[0].slots)
    assert base - no_ls == {f"{PREFIX}transformer.resblocks.{j}.ls_{i}.gamma" for j in (0, 1) for i in (1, 2)}
    st, pooled = cpu_tower(tiny_config(g, pool_type="tok"))
    assert sorted(pooled.unused_parameter_names()) == sorted(n for n in st.slots if "vit_downsampler" in n)


@pytest.mark.parametrize("grid,tokens", [(4, 1), (6, 4), (8, 4), (52, 169)])
def test_num_patches_is_the_true_count_after_two_stride_2_convolutions(golden_dir, grid, tokens):
    """T -> (T - 1) // 2 + 1, twice.  Equal to the reference's (grid // 4) ** 2 wherever the grid divides by 4 (4, 8, 52); grid 6
    gives 6 -> 3 -> 2, four tokens, where the reference's property says one"""
    from dexbotic_amd.model.modules.mm_vision.pe import PEVisionTower
    assert PEVisionTower.tokens_out(grid) == tokens
    if grid % 4 == 0:
        assert tokens == (grid // 4) ** 2
    if grid <= 8:
        assert cpu_tower(tiny_config(load(golden_dir), image_size=4 * grid))[1].num_patches == tokens


def test_builder_dispatches_on_name_and_on_config(golden_dir):
    from dexbotic_amd.engine import ParamStore, building
    from dexbotic_amd.model.modules.mm_vision.builder import build_vision_tower
    from dexbotic_amd.model.modules.mm_vision.pe import PEVisionTower
    g = load(golden_dir)
    cfg = tiny_config(g)
    assert isinstance(build_vision_tower(cfg, ParamStore("cpu", torch.float32)), PEVisionTower)
    assert isinstance(build_vision_tower(cfg.to_dict(), ParamStore("cpu", torch.float32)), PEVisionTower)

    class Carrier:
        mm_vision_tower = cfg
    with building(ParamStore("cpu", torch.float32)):
        assert isinstance(build_vision_tower(Carrier()), PEVisionTower)
    # the registered name: the real tower (only registered, nothing is allocated before finalize)
    st = ParamStore("cpu", torch.float32)
    t = build_vision_tower("pe_lang_l14_728", st)
    assert isinstance(t, PEVisionTower) and (t.hidden_size, t.num_patches, len(t.layer_specs)) == (1024, 169, 23)
    assert st.slots[PREFIX + "positional_embedding"].shape == (2705, 1024)
    assert st.slots[PREFIX + "vit_downsampler2.weight"].shape == (4096, 2048, 3, 3)
    with pytest.raises(ValueError, match="Unknown configuration name"):
        build_vision_tower("pe_core_g14", ParamStore("cpu", torch.float32))


def test_unsupported_options_are_refused_by_name(golden_dir):
    g = load(golden_dir)
    with pytest.raises(NotImplementedError, match="pool_type='attn'"):
        cpu_tower(tiny_config(g, pool_type="attn"))
    with pytest.raises(ValueError, match="pool_type"):
        cpu_tower(tiny_config(g, pool_type="max"))
    with pytest.raises(ValueError, match="use_rope2d"):
        cpu_tower(tiny_config(g, use_rope2d=False))
    with pytest.raises(NotImplementedError, match="use_abs_posemb"):
        cpu_tower(tiny_config(g, use_abs_posemb=False))
    with pytest.raises(ValueError, match="multiple of 4"):
        cpu_tower(tiny_config(g, width=60, heads=2))


def test_image_processor_is_siglip_at_image_size_with_half_mean_and_std(golden_dir):
    proc = cpu_tower(tiny_config(load(golden_dir)))[1].image_processor
    assert dict(proc.size) == {"height": 24, "width": 24}
    assert list(proc.image_mean) == [0.5, 0.5, 0.5] and list(proc.image_std) == [0.5, 0.5, 0.5]
    assert proc.do_resize and proc.do_rescale and proc.do_normalize and abs(proc.rescale_factor - 1 / 255) < 1e-12


def test_rope_tables_follow_the_written_out_formula():
    """first D/2 columns turn with the column index, the last D/2 with the row index, each frequency twice, +1 with a CLS token whose
    own row is zero; another grid picks rows r * max_w + c of the native table"""
    from dexbotic_amd import kernels as K
    D, G = 16, 6
    cos_t, sin_t = K.rope2d_tables(G, G, D, G, G, True, "cpu")
    assert tuple(cos_t.shape) == (G * G + 1, D) and cos_t.dtype == torch.float32
    assert torch.equal(cos_t[0], torch.ones(D)) and torch.equal(sin_t[0], torch.zeros(D))
    inv = 10000.0 ** -(np.arange(0, D // 2, 2) / (D // 2))
    r, c = 4, 2
    ang = np.concatenate([np.repeat((c + 1) * inv, 2), np.repeat((r + 1) * inv, 2)])
    np.testing.assert_allclose(cos_t[1 + r * G + c].numpy(), np.cos(ang), atol=1e-6)
    np.testing.assert_allclose(sin_t[1 + r * G + c].numpy(), np.sin(ang), atol=1e-6)
    pc, ps = K.rope2d_tables(3, 2, D, G, G, True, "cpu")
    assert tuple(pc.shape) == (7, D)
    for i, (rr, cc) in enumerate((a, b) for a in range(3) for b in range(2)):
        assert torch.equal(pc[1 + i], cos_t[1 + rr * G + cc]) and torch.equal(ps[1 + i], sin_t[1 + rr * G + cc])
    nc, _ = K.rope2d_tables(2, 2, D, 2, 2, False, "cpu")
    assert tuple(nc.shape) == (4, D) and torch.equal(nc[0], torch.ones(D))          # position (0, 0) without the CLS shift


def test_weight_recipe_reproduces_the_stored_checksums(golden_dir):
    for name in ("pe_t1.npz", "dm0_pe_t1.npz"):
        g = np.load(os.path.join(golden_dir, name), allow_pickle=False)
        w, images = PW.from_fixture(g)
        keys = [str(k) for k in g["w_keys"]]
        np.testing.assert_allclose(MW.checksums(keys, w), g["w_checksums"], rtol=1e-12, atol=1e-9)
        np.testing.assert_allclose(MW.checksums(["images"], {"images": images}), g["image_checksum"], rtol=1e-12, atol=1e-9)
        gam = [k for k in keys if k.endswith(".gamma")]
        assert len(gam) == 4 and all(abs(float(w[k].mean()) - 1.0) < 0.3 for k in gam)     # order 1, not 0.05


def test_new_entry_points_are_in_the_header_and_the_ctypes_table():
    from dexbotic_amd import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dexbotic_amd.h")).read(), flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", src), s
        assert s in L.SIGNATURES and hasattr(L.lib, s), s
    assert L.lib.dxa_layerscale_bwd_rows(1) == 4 and L.lib.dxa_layerscale_bwd_rows(8115) == 1024


def test_dm0_config_with_the_tower_round_trips_and_the_keys_equal_the_references(golden_dir, tmp_path):
    from dexbotic_amd.model import DM0Config, DM0ForCausalLM
    from .test_pe_gpu import dm0_config
    g = np.load(os.path.join(golden_dir, "dm0_pe_t1.npz"), allow_pickle=False)
    c = dm0_config(g)
    c.save_pretrained(str(tmp_path))
    c2 = DM0Config.from_pretrained(str(tmp_path))
    assert c2.to_dict() == c.to_dict()
    m = DM0ForCausalLM(c2, device="cpu", train=False)
    want = dict(zip((str(k) for k in g["w_keys"]), MW.unpack_shapes(g["w_shapes"])))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert want["model.mm_projector.weight"] == (96, 256) and "model.mm_projector.bias" not in want
    assert sorted(m.unused_parameter_names()) == sorted(str(n) for n in g["no_grad"])
