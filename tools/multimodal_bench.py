#!/usr/bin/env python
"""The multi_modal cross-attention (gnpde_cross_attention_f32 through ops.cross_attention)
against its torch restatement (ops.cross_attention_torch: the [B, N, M] scores materialised)
on the same device, in ONE process, and the whole multi_modal RHS at the first size.

Sizes: ogbn-arxiv's rows at G-arxiv's width (R = 169,343, C = 128) against M = 64, 256 and
1,024 tokens; a Cora-sized graph (N = 2,485, C = 80, M = 256); a batch of image-sized graphs
(B = 64, N = M = 196, C = 128).  Standard normal q / k / v from a seed, scale = 1 / sqrt(C).

Per case: both paths between HIP events after warm-up (median / min / max of --reps calls),
their ratio, the achieved FLOP/s of the kernel counted as 4 R M C (the two products) against
the fp32 matrix-core peak of 157.3 TFLOP/s, the peak device memory each path allocates on
top of its inputs (torch.cuda.max_memory_allocated around one call: the scratch), and the
two results compared at the size timed.  The RHS case times MultiModalLaplacianODEFunc's
no-grad forward on the G-arxiv graph (q projection, cross-attention, K1; k / v cached) and
the same with the torch restatement in the kernel's place.

Prints one JSON document (--out FILE also writes it).  No GPU: it fails (nothing to measure)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-pde_amd"))
import torch  # noqa: E402

import gnpde  # noqa: E402
from gnpde import ops, synthetic  # noqa: E402

PEAK_FLOPS = 157.3e12  # fp32 matrix cores (v_mfma_f32_32x32x2_f32), MI355X
CASES = {
    "arxiv_m64": (1, 169343, 64, 128),
    "arxiv_m256": (1, 169343, 256, 128),
    "arxiv_m1024": (1, 169343, 1024, 128),
    "cora_m256": (1, 2485, 256, 80),
    "batch64_196": (64, 196, 196, 128),
}
RHS_CASE = "arxiv_m64"
D2 = 64  # the second modality's width in the RHS case


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "reps": reps}


def scratch_bytes(fn):
    """Peak device memory one call holds on top of what is allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    nbytes = sum(t.numel() * t.element_size() for t in (out if isinstance(out, tuple) else (out,)))
    del out
    return {"peak_bytes": int(peak), "beyond_output_bytes": int(peak - nbytes)}


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def rhs_case(B, N, M, C, dev, warmup, reps):
    opt = {'hidden_dim': C, 'block': 'constant', 'function': 'laplacian', 'add_source': True,
           'no_alpha_sigmoid': False, 'max_nfe': 10 ** 9, 'multi_modal': True, 'gnpde_multi_modal': True,
           'second_modality_dim': D2}
    func = gnpde.set_function(opt)(C, C, opt, dev).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(3)
    with torch.no_grad():
        for lin in (func.Q2, func.K2, func.V2):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=gen, device=dev) * 0.1)
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=gen, device=dev) * 0.1)
        func.alpha_train.fill_(0.3)
        func.beta_train.fill_(0.7)
    ei, w = synthetic.rw_graph(N, synthetic.ARXIV_E, seed=0, device=dev)
    func.edge_index, func.edge_weight = ei, w
    x = synthetic.features(B, N, C, seed=1, device=dev)
    func.x0 = x.clone()
    func.y = torch.randn(B, M, D2, generator=gen, device=dev)
    t = torch.tensor(0.0)

    def composed():
        Wq, bq = func.q_params()
        k, v = func.kv(func.y)
        xt = ops.cross_attention_torch(ops.linear(x, Wq, bq)[0].view(x.shape), k, v, func.scale)
        g = func.graph_for(x)
        return ops.spmm_rhs(g, func.csr_weights(g, w, 'w'), xt, x0=func.x0, alpha=func.alpha_train.detach(),
                            beta=func.beta_train.detach(), rhs=True, alpha_sigmoid=True, add_source=True)

    with torch.no_grad():
        kern = timed(lambda: func(t, x), warmup, reps)
        base = timed(composed, warmup, reps)
        err = relerr(func(t, x), composed())
    return {"rows": B * N, "width": C, "tokens": M, "second_modality_dim": D2, "edges": int(ei.shape[2]),
            "rhs_ms": kern, "rhs_torch_attention_ms": base, "torch_over_kernel": base["median"] / kern["median"],
            "rel_diff": err}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-rhs", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("multimodal_bench: no GPU, nothing to measure")
    if args.reps < 10:
        sys.exit("multimodal_bench: --reps must be at least 10")
    dev = "cuda:0"
    doc = {"device": torch.cuda.get_device_name(0), "build_id": gnpde.build_info()["build_id"],
           "peak_flops": PEAK_FLOPS, "cases": {}}
    for name in args.cases.split(","):
        B, N, M, C = CASES[name]
        print(name, file=sys.stderr, flush=True)
        gen = torch.Generator(device=dev).manual_seed(1)
        q = torch.randn(B, N, C, generator=gen, device=dev)
        k = torch.randn(B, M, C, generator=gen, device=dev)
        v = torch.randn(B, M, C, generator=gen, device=dev)
        scale = 1.0 / C ** 0.5
        kern = timed(lambda: ops.cross_attention(q, k, v, scale), args.warmup, args.reps)
        base = timed(lambda: ops.cross_attention_torch(q, k, v, scale), args.warmup, args.reps)
        flops = 4.0 * B * N * M * C
        doc["cases"][name] = {
            "B": B, "N": N, "M": M, "C": C, "rows": B * N,
            "kernel_ms": kern, "torch_ms": base, "torch_over_kernel": base["median"] / kern["median"],
            "kernel_tflops": flops / (kern["median"] * 1e-3) / 1e12,
            "kernel_fraction_of_peak": flops / (kern["median"] * 1e-3) / PEAK_FLOPS,
            "torch_tflops": flops / (base["median"] * 1e-3) / 1e12,
            "kernel_scratch": scratch_bytes(lambda: ops.cross_attention(q, k, v, scale)),
            "torch_scratch": scratch_bytes(lambda: ops.cross_attention_torch(q, k, v, scale)),
            "score_buffer_bytes": 4 * B * N * M,
            "rel_diff": relerr(ops.cross_attention(q, k, v, scale), ops.cross_attention_torch(q, k, v, scale)),
        }
        del q, k, v
        torch.cuda.empty_cache()
    if not args.no_rhs:
        print("rhs", file=sys.stderr, flush=True)
        doc["rhs"] = rhs_case(*CASES[RHS_CASE], dev, args.warmup, args.reps)
    out = json.dumps(doc, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
