#!/usr/bin/env python
"""The Perception Encoder tower at its real size (pe_lang_l14_728: 728 px / patch 14 = 2705 tokens, width 1024, 23 blocks, 16 heads x 64,
two stride-2 convolutions down to 169 tokens of 4096 columns) in bf16 with random weights, and each of its new kernels at the
production shape against the same arithmetic in eager torch ops on the same GPU.  Device events, one process, the candidates
alternating round by round; median, min and max over the rounds.

    python scripts/pe_bench.py [--out out.txt]         tower forward and forward + backward for 1 and 3 images, then the kernels
    python scripts/pe_bench.py --trace                 five forward + backward steps of 3 images and nothing else: the run to put
                                                       under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --`
    python scripts/pe_bench.py --share DIR [--out f]   per-kernel share of that run from DIR's *kernel_stats.csv (appended to f)
"""
import argparse
import csv
import glob
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda"
ROUNDS = 7


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps           # us per call


def alternate(fns, reps, rounds=ROUNDS):
    for f in fns.values():
        timed(f, 2)                                    # warm up every shape
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            t[k].append(timed(f, reps))
    return t


def row(name, v, note=""):
    med = statistics.median(v)
    return f"  {name:34s} median {med:10.1f} us  min {min(v):10.1f}  max {max(v):10.1f}  spread {(max(v) - min(v)) / med * 100:5.1f} %{note}"


def build_tower():
    from dexbotic_amd.engine import ParamStore, attach_parameters
    from dexbotic_amd.model.modules.mm_vision.builder import build_vision_tower
    st = ParamStore(DEV, torch.bfloat16)
    tower = build_vision_tower("pe_lang_l14_728", st)
    st.finalize(train=True)
    attach_parameters(tower, st)
    torch.manual_seed(0)
    st.master.normal_(0.0, 0.02)
    for n in st.slots:
        leaf = n.rsplit(".", 1)[-1]
        if leaf == "gamma":
            st.w32(n).fill_(0.1)
        elif leaf == "weight" and len(st.slots[n].shape) == 1:
            st.w32(n).fill_(1.0)
    st.sync_shadow()
    return st, tower


def tower_flops(n_img):
    """forward FLOPs from the shapes: the GEMMs of the blocks, attention, patch embedding and the two convolutions"""
    T, C, I, L, g = 2705, 1024, 4096, 23, 52
    blk = 2 * T * C * (3 * C + C + 2 * I) + 4 * T * T * C
    conv = 2 * 26 * 26 * 9 * C * 2 * C + 2 * 13 * 13 * 9 * 2 * C * 4 * C
    return n_img * (L * blk + 2 * g * g * 588 * C + conv)


def tower_steps(st, tower, n_img):
    torch.manual_seed(1)
    images = torch.randn(n_img, 3, 728, 728, device=DEV)
    dy = torch.randn(n_img, 169, 4096, device=DEV).bfloat16()

    def fwd():
        with torch.no_grad():
            return tower(images)

    def fwd_bwd():
        st.begin_step()
        tower(images).backward(dy)
    return fwd, fwd_bwd


def bench_tower(lines):
    st, tower = build_tower()
    n_par = sum(s.numel for s in st.slots.values())
    lines.append(f"tower pe_lang_l14_728, bf16, random weights, {n_par / 1e6:.1f} M parameters; activations kept (no recompute)")
    for n_img in (1, 3):
        fwd, fwd_bwd = tower_steps(st, tower, n_img)
        out = fwd()
        assert tuple(out.shape) == (n_img, 169, 4096) and bool(torch.isfinite(out.float()).all())
        t = alternate({"forward": fwd, "forward + backward": fwd_bwd}, reps=3, rounds=5)
        fl = tower_flops(n_img)
        for k, v in t.items():
            mult = 1 if k == "forward" else 3
            lines.append(row(f"{n_img} image(s) {k}", v, f"   ({mult * fl / 1e12:.2f} TFLOP from the shapes -> "
                                                         f"{mult * fl / statistics.median(v) / 1e6:.0f} TFLOP/s whole-tower rate)"))
        lines.append(f"    peak memory allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    del st, tower
    torch.cuda.empty_cache()


def bench_kernels(lines):
    from dexbotic_amd import kernels as K
    torch.manual_seed(2)
    N, T, H, D, C = 3, 2705, 16, 64, 1024
    M = N * T
    lines.append("")
    lines.append("kernels at the production shape against eager torch ops computing the same thing (bf16)")
    # ---- rotation of q and k in the packed projection [3 x 2705, 3, 16, 64]
    qkv = torch.randn(M, 3 * C, device=DEV).bfloat16()
    cos_t, sin_t = K.rope2d_tables(52, 52, D, 52, 52, True, DEV)
    c5, s5 = cos_t[None, :, None, :], sin_t[None, :, None, :]

    def eager_rope():
        q5 = qkv.view(N, T, 3, H, D)
        out = []
        for i in (0, 1):
            t = q5[:, :, i].float()
            rot = torch.stack((-t[..., 1::2], t[..., 0::2]), -1).flatten(-2)
            out.append((t * c5 + rot * s5).to(torch.bfloat16))
        return out
    ours = K.rope2d_(qkv.clone(), cos_t, sin_t, N, T, H, D).view(N, T, 3, H, D)
    ref = eager_rope()
    d = max((ours[:, :, i].float() - ref[i].float()).abs().max().item() for i in (0, 1))
    byt = M * 2 * C * 2 * 2
    t = alternate({"dxa_rope2d_fwd (in place)": lambda: K.rope2d_(qkv, cos_t, sin_t, N, T, H, D),
                   "dxa_rope2d_bwd (in place)": lambda: K.rope2d_(qkv, cos_t, sin_t, N, T, H, D, backward=True),
                   "eager rotate q and k": eager_rope}, reps=20)
    lines.append(f" rotation [3 x 2705, 3, 16, 64]: max |ours - eager| {d:.3e}; bytes needed {byt / 1e6:.0f} MB (q and k read and written)")
    for k, v in t.items():
        lines.append(row(k, v, f"   {byt / statistics.median(v) / 1e6:.2f} TB/s" if k.startswith("dxa") else ""))
    # ---- scaled add [3 x 2705, 1024]
    x, h, dy = (torch.randn(M, C, device=DEV).bfloat16() for _ in range(3))
    gamma = (1 + 0.5 * torch.randn(C, device=DEV)).bfloat16()

    def ours_ls_bwd():
        dh, part = K.layerscale_residual_bwd(dy, h, gamma)
        return dh, K.colsum(part)

    def eager_ls_bwd():
        return dy * gamma, (dy.float() * h.float()).sum(0)
    d = (K.layerscale_residual_fwd(x, h, gamma).float() - (x + gamma * h).float()).abs().max().item()
    dg = (ours_ls_bwd()[1] - eager_ls_bwd()[1]).abs().max().item()
    t = alternate({"dxa_layerscale_residual_fwd": lambda: K.layerscale_residual_fwd(x, h, gamma),
                   "eager x + gamma * h": lambda: x + gamma * h,
                   "dxa_layerscale_residual_bwd + colsum": ours_ls_bwd, "eager dy * gamma, sum(dy * h)": eager_ls_bwd}, reps=20)
    b1 = M * C * 2
    need = {"dxa_layerscale_residual_fwd": 3 * b1, "dxa_layerscale_residual_bwd + colsum": 3 * b1}
    lines.append(f" scaled add [3 x 2705, 1024]: max |ours - eager| fwd {d:.3e} (eager rounds gamma * h to bf16 first), dgamma {dg:.3e}; "
                 "no LayerNorm-fused variant is built")
    for k, v in t.items():
        lines.append(row(k, v, f"   {need[k] / statistics.median(v) / 1e6:.2f} TB/s over {need[k] / 1e6:.0f} MB" if k in need else ""))
    # ---- the two convolutions: 52 -> 26 at 1024 -> 2048 channels, 26 -> 13 at 2048 -> 4096
    for Tg, Ci in ((52, C), (26, 2 * C)):
        try:
            bench_conv(lines, K, N, Tg, Ci)
        except RuntimeError as e:                   # (the eager side's library refusing the shape is a result, not a crash)
            lines.append(f" convolution at grid {Tg}, {Ci} channels did not run: {type(e).__name__}: {str(e)[:300]}")


def bench_conv(lines, K, N, Tg, Ci):
    Co, To = 2 * Ci, K.conv_out_grid(Tg)
    xt = torch.randn(N, Tg * Tg, Ci, device=DEV).bfloat16()
    w = (torch.randn(Co, Ci, 3, 3, device=DEV) * (9 * Ci) ** -0.5).bfloat16()
    b = torch.randn(Co, device=DEV).bfloat16()
    dyc = torch.randn(N * To * To, Co, device=DEV).bfloat16()
    w2 = w.view(Co, 9 * Ci)

    def ours_fwd():
        return K.mm_nt(K.conv3x3s2_im2col(xt, Tg), w2, bias=b)

    def eager_fwd():
        y = F.conv2d(xt.transpose(1, 2).reshape(N, Ci, Tg, Tg), w, b, stride=2, padding=1)
        return y.view(N, Co, To * To).transpose(1, 2).contiguous()
    rows = K.conv3x3s2_im2col(xt, Tg)

    def ours_bwd():
        dw = K.mm_tn(dyc, rows, out_dtype=torch.float32)
        db = K.colsum(dyc)
        return K.conv3x3s2_col2im(K.mm_nn(dyc, w2), N, Tg), dw, db
    xg, wg, bg = xt.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)

    def eager_fwd_bwd():
        y = F.conv2d(xg.transpose(1, 2).reshape(N, Ci, Tg, Tg), wg, bg, stride=2, padding=1)
        return torch.autograd.grad(y, (xg, wg, bg), dyc.view(N, To, To, Co).permute(0, 3, 1, 2))
    d = (ours_fwd().float().view(N, To * To, Co) - eager_fwd().float()).abs().max().item()
    dxo, dxe = ours_bwd()[0].float(), eager_fwd_bwd()[0].float()
    t = alternate({"dxa_conv3x3s2_im2col + dxa_gemm": ours_fwd, "eager F.conv2d": eager_fwd,
                   "ours fwd + bwd (dX, dW, db)": lambda: (ours_fwd(), ours_bwd()), "eager conv2d fwd + bwd": eager_fwd_bwd,
                   "dxa_conv3x3s2_im2col alone": lambda: K.conv3x3s2_im2col(xt, Tg),
                   "dxa_conv3x3s2_col2im alone": lambda: K.conv3x3s2_col2im(rows, N, Tg)}, reps=5)
    fl = 2 * N * To * To * 9 * Ci * Co
    lines.append(f" convolution {Tg} -> {To}, {Ci} -> {Co} channels, 3 images: max |ours - eager| fwd {d:.3e}, dX {(dxo - dxe).abs().max().item():.3e}; "
                 f"{fl / 1e9:.0f} GFLOP forward")
    for k, v in t.items():
        note = f"   {fl / statistics.median(v) / 1e6:.0f} TFLOP/s" if k in ("dxa_conv3x3s2_im2col + dxa_gemm", "eager F.conv2d") else ""
        lines.append(row(k, v, note))


def trace():
    st, tower = build_tower()
    _, fwd_bwd = tower_steps(st, tower, 3)
    for _ in range(5):
        fwd_bwd()
    torch.cuda.synchronize()


def share(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        sys.exit(f"pe_bench --share: no *kernel_stats.csv under {d}")
    rows = list(csv.DictReader(open(files[0])))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    lines = ["", f"per-kernel share of five forward + backward steps of 3 images (rocprofv3 --kernel-trace --stats, a run of its own; "
                 f"{tot / 5e6:.1f} ms of kernel time per step, build and warm-up launches included in the totals)"]
    rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
    for r in rows[:18]:
        lines.append(f"  {float(r['TotalDurationNs']) / tot * 100:5.1f} %  {int(r['Calls']):6d} calls  {float(r['AverageNs']) / 1e3:9.1f} us avg  {r['Name'][:110]}")
    new = [r for r in rows if any(s in r["Name"] for s in ("rope2d_k", "layerscale_residual", "conv3x3s2"))]
    lines.append(f"  the new kernels together: {sum(float(r['TotalDurationNs']) for r in new) / tot * 100:.2f} %")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--share")
    a = ap.parse_args()
    if a.share:
        lines = share(a.share)
        mode = "a"
    else:
        if not torch.cuda.is_available():
            sys.exit("pe_bench: needs the GPU (no timing is taken on a CPU)")
        if a.trace:
            return trace()
        lines = [__doc__.split("\n\n")[0], "", f"us per call, device events, {ROUNDS} alternating rounds (5 for the tower); spread = (max - min) / median over the rounds", ""]
        bench_tower(lines)
        bench_kernels(lines)
        mode = "w"
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, mode) as f:
            f.write(text)


if __name__ == "__main__":
    main()
