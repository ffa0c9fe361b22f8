"""MLP2, the ViT out-projection and their producers, SPLIT3 form against HALF2-chain form, in one process:
interleaved rounds, median per call, at the 512^2 batch-8 shapes (M = 32768 tokens).

  mlp2      ops.linear_split3 on bf16 planes against ops.linear_half2_planes on fp16 planes, K0 = 2048, N = 512,
            with the residual
  out_proj  the same at K0 = N = 512 with the residual
  mlp1      the HALF2 MLP1 (K0 = 512, N = 2048, ReLU) writing three bf16 planes against two fp16 planes
  vit_attn  the batch-axis attention (L = 8, ntok = 4096) storing three bf16 planes against two fp16 planes
Each pair is also timed A against A (the SPLIT3-side form against its own second copy): that difference is
the resolution of the comparison.

    python tools/half2_chain_ab.py [rounds] [iters]
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mhada-style-transfer_amd")]

import torch

from mhada_hip import ops
from proj_split3_ab import ab


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    torch.manual_seed(0)
    dev = "cuda"
    M, C, H, heads = 32768, 512, 2048, 8
    g, be = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.3
    x = torch.randn(M, C, device=dev) * 2
    r = torch.randn(M, C, device=dev)
    w1, b1 = torch.randn(H, C, device=dev) / C ** 0.5, torch.randn(H, device=dev)
    w2, b2 = torch.randn(C, H, device=dev) / H ** 0.5, torch.randn(C, device=dev)
    wq, bq = torch.randn(3 * C, C, device=dev) / C ** 0.5, torch.randn(3 * C, device=dev) * 0.3
    wo, bo = torch.randn(C, C, device=dev) / C ** 0.5, torch.randn(C, device=dev)
    h1, hq = ops.half2_prepare(g, be, w1), ops.half2_prepare(g, be, wq)
    hm, ho = ops.half2_chain_prepare(g, be, w1, b1, w2), ops.half2_chain_prepare(g, be, wq[2 * C:], bq[2 * C:], wo)
    pl = ops.layernorm_half2(x, g, be, 1e-6, h1["s_a"])

    def mlp1(**kw):
        return ops.linear_half2(pl, h1["w2"], h1["cs"], b1, torch.float32, relu=True, out_planes=True, **kw)
    m3, m2 = mlp1(), mlp1(out_scale=hm["u"])
    w6 = ops.split3_weight(w2)
    ab("mlp2", {"split3": lambda: ops.linear_split3(m3, w6, b2, torch.float32, residual=r),
                "split3'": lambda: ops.linear_split3(m3, w6, b2, torch.float32, residual=r),
                "half2": lambda: ops.linear_half2_planes(m2, hm["w2"], hm["cs"], b2, residual=r)}, rounds, iters)
    del m3, m2
    L, ntok = 8, M // 8
    qkv = ops.linear_half2(ops.layernorm_half2(x, g, be, 1e-6, hq["s_a"]), hq["w2"], hq["cs"], bq, torch.float32)
    qkv = qkv.view(L, ntok, 3 * C)
    a3, a2 = ops.vit_batch_attn_split3(qkv, L, ntok, heads), ops.vit_batch_attn_half2(qkv, L, ntok, heads, ho["u"])
    wo6 = ops.split3_weight(wo)
    ab("out_proj", {"split3": lambda: ops.linear_split3(a3, wo6, bo, torch.float32, residual=r),
                    "split3'": lambda: ops.linear_split3(a3, wo6, bo, torch.float32, residual=r),
                    "half2": lambda: ops.linear_half2_planes(a2, ho["w2"], ho["cs"], bo, residual=r)}, rounds, iters)
    ab("mlp1", {"bf16x3": mlp1, "bf16x3'": mlp1, "fp16x2": lambda: mlp1(out_scale=hm["u"])}, rounds, iters)
    ab("vit_attn", {"bf16x3": lambda: ops.vit_batch_attn_split3(qkv, L, ntok, heads),
                    "bf16x3'": lambda: ops.vit_batch_attn_split3(qkv, L, ntok, heads),
                    "fp16x2": lambda: ops.vit_batch_attn_half2(qkv, L, ntok, heads, ho["u"])}, rounds, iters)


if __name__ == "__main__":
    main()
