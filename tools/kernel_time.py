"""Stand-alone HIP-event times of single kernels at the shapes of the B = 64 fusion step, one
registered case per kernel family.  A case declares, for a batch B, its shapes with their
algorithmic bytes or FLOPs (the plan) and a run that allocates the inputs, times the launches
through _harness.time_us and prints the case's result lines.

  python tools/kernel_time.py <case>... | --all  [--batch 64] [--iters N] [--tag product]
  python tools/kernel_time.py --list             the case names
  python tools/kernel_time.py --plan <case>...   shapes and algorithmic work; needs no GPU

DFU_HIP_LIB selects another build of the library for an A/B (tools/build_exp.sh); `ln_fwd` and
`epi` run on seeded inputs and print output checksums, so two builds compare bit for bit.
"""
import argparse

import _harness
import torch
from _harness import VIT_SHAPES, lib_tag, time_us

from dfu_hip import _lib as L
from dfu_hip import ops

CASES = {}  # name -> (case function, default iterations, unit of the plan's work)


def case(iters, unit):
    def reg(fn):
        CASES[fn.__name__] = (fn, iters, unit)
        return fn
    return reg


def _bf(*shape, scale=None):
    """Random bf16 operand; no scaling pass (and no fp32 temporary of it) unless asked for."""
    x = torch.randn(*shape, device="cuda")
    return (x if scale is None else x * scale).to(torch.bfloat16)


@case(20, "B")
def adamw(B):
    """The flat AdamW kernel at the fusion model's parameter count.  Bytes per parameter: p, g,
    m, v read (16) + p, m, v written (12) + the bf16 shadow (2)."""
    n = 110_750_000

    def run(iters, tag):
        p, g = torch.randn(n, device="cuda"), torch.randn(n, device="cuda")
        m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        sh = torch.empty(n, dtype=torch.bfloat16, device="cuda")
        step = torch.ones((), dtype=torch.int64, device="cuda")
        us = time_us(lambda: ops.adamw_flat(p, g, m, v, 1e-4, 0.9, 0.999, 1e-8, 1e-4, step, sh),
                     iters, 3, sync=False)
        print(f"adamw_flat n={n}: {us:.1f} us, {30 * n / us / 1e3:.0f} GB/s algorithmic")
    return [(f"n={n}", 30 * n)], run


@case(50, "FLOP")
def attn(B):
    """The attention kernels at the ViT-B/16 shape: forward (bf16, fp16, bf16x3) and the fused
    backward.  FLOPs: forward 4 N^2 dh per head, backward 2.5x."""
    N, H, dh = 197, 12, 64
    fl = 4.0 * N * N * dh * B * H

    def run(iters, tag):
        qkv = _bf(B * N, 3 * H * dh, scale=0.5)
        dout = _bf(B * N, H * dh, scale=0.1)
        scale = dh ** -0.5
        o, lse = ops.attention_fwd(qkv, B, N, H, dh, scale)
        dq = torch.empty_like(qkv)
        tf = time_us(lambda: ops.attention_fwd(qkv, B, N, H, dh, scale), iters, 3)
        tb = time_us(lambda: ops.attention_bwd(qkv, o, dout, lse, B, N, H, dh, scale, dq), iters, 3)
        qf, qb = qkv.float(), torch.empty_like(qkv)
        tx = time_us(lambda: ops.attention_fwd_f32(qf, B, N, H, dh, scale, qkv_bf16=qb), iters, 3)
        q16 = qkv.to(torch.float16)
        th = time_us(lambda: ops.attention_fwd_f16(q16, B, N, H, dh, scale), iters, 3)
        print(f"attention fwd {tf:.1f} us ({fl / tf / 1e6:.0f} TFLOP/s)  fwd fp16 {th:.1f} us  bwd "
              f"{tb:.1f} us ({2.5 * fl / tb / 1e6:.0f} TFLOP/s)  fwd bf16x3 {tx:.1f} us")
    shape = f"B={B} N={N} H={H} dh={dh}"
    return [(f"fwd {shape}", fl), (f"bwd {shape}", 2.5 * fl)], run


@case(50, "B")
def bn_apply(B):
    """dfu_bn_apply (BN scale/shift + residual + ReLU, bf16 NHWC) at the ResNet-50 shapes
    (DFU_BN_BLOCKS caps the grid for sweeps).  Bytes: y read + residual read (if any) + out
    written, 2 each per element."""
    shapes = [(B * 112 * 112, 64, False), (B * 56 * 56, 64, False), (B * 56 * 56, 256, True),
              (B * 28 * 28, 512, True), (B * 14 * 14, 1024, True), (B * 7 * 7, 2048, True)]
    nbytes = lambda M, C, res: M * C * 2 * (3 if res else 2)  # noqa: E731

    def run(iters, tag):
        tot = 0.0
        for M, C, res in shapes:
            y = _bf(M, C)
            r = _bf(M, C) if res else None
            out = torch.empty_like(y)
            sc, sh = torch.rand(C, device="cuda"), torch.rand(C, device="cuda")
            us = time_us(lambda: ops.bn_apply(y, sc, sh, r, True, out, M, C), iters, 3, sync=False)
            tot += us
            print(f"bn_apply M={M} C={C} res={res}: {us:.1f} us, "
                  f"{nbytes(M, C, res) / us / 1e3:.0f} GB/s")
        print(f"total {tot:.1f} us")
    return [(f"M={M} C={C} res={res}", nbytes(M, C, res)) for M, C, res in shapes], run


@case(50, "B")
def bn_apply_x3(B):
    """dfu_bn_apply_x3 (the parity mode's BN apply over split pairs) at the step's ResNet-50
    shapes: conv output pair in, optional residual pair, out pair + ReLU bitmask.  Bytes per
    element: 4 (y pair) [+ 4 residual pair] + 4 (out pair) + 1/8 (mask)."""
    # (rows, C, residual pair?, count per step): bn1/bn2 (no residual) and bn3 (+ residual pair)
    shapes = [(B * 56 * 56, 64, False, 6), (B * 56 * 56, 256, True, 3),
              (B * 28 * 28, 128, False, 7), (B * 28 * 28, 512, True, 4),
              (B * 14 * 14, 256, False, 11), (B * 14 * 14, 1024, True, 6),
              (B * 7 * 7, 512, False, 5), (B * 7 * 7, 2048, True, 3)]
    nbytes = lambda M, C, res: M * C * ((8 if res else 4) + 4 + 0.125)  # noqa: E731

    def run(iters, tag):
        tot_us = tot_b = 0.0
        for M, C, res, cnt in shapes:
            y, ylo = _bf(M, C), _bf(M, C, scale=1e-3)
            r = _bf(M, C) if res else None
            rlo = _bf(M, C, scale=1e-3) if res else None
            out, lo = torch.empty_like(y), torch.empty_like(y)
            mask = torch.empty(M * C // 8, dtype=torch.uint8, device="cuda")
            sc, sh = torch.rand(C, device="cuda"), torch.rand(C, device="cuda")
            us = time_us(lambda: ops.bn_apply_x3(y, sc, sh, r, 2 if res else 0, True, M, C,
                                                 out_lo=lo, out_bf16=out, residual_lo=rlo,
                                                 y_lo=ylo, relu_mask=mask), iters, 3, sync=False)
            nb = nbytes(M, C, res)
            tot_us += us * cnt
            tot_b += nb * cnt
            print(f"M={M:7d} C={C:5d} res={int(res)}: {us:7.1f} us  {nb / us / 1e3:6.0f} GB/s  "
                  f"(x{cnt})", flush=True)
        print(f"per step: {tot_us / 1e3:.3f} ms, {tot_b / 1e9:.2f} GB, "
              f"{tot_b / tot_us / 1e3:.0f} GB/s")
    return [(f"M={M} C={C} res={int(res)} x{cnt}", nbytes(M, C, res))
            for M, C, res, cnt in shapes], run


@case(30, "B")
def bn_bwd(B):
    """The BatchNorm backward (reduce -> finalize -> apply) at the ResNet-50 shapes.  Bytes:
    reduce reads dout, y (+ out for the residual mask); apply reads the same and writes dy
    (+ dres); 2 per element each."""
    # (M, C, relu mode, residual): conv1/conv2 BN+ReLU recompute the mask (2); block output BN +
    # residual + ReLU masks from the stored output (1) and emits dres
    shapes = [(B * 112 * 112, 64, 2, False), (B * 56 * 56, 64, 2, False),
              (B * 56 * 56, 256, 1, True), (B * 28 * 28, 128, 2, False),
              (B * 28 * 28, 512, 1, True), (B * 14 * 14, 256, 2, False),
              (B * 14 * 14, 1024, 1, True), (B * 7 * 7, 512, 2, False),
              (B * 7 * 7, 2048, 1, True)]

    def nbytes(M, C, relu, res):
        nrd = 3 if relu == 1 else 2
        return M * C * 2 * (2 * nrd + 1 + (1 if res else 0))

    def run(iters, tag):
        tot = 0.0
        for M, C, relu, res in shapes:
            dout, y = _bf(M, C), _bf(M, C)
            out = torch.relu(torch.randn(M, C, device="cuda")).to(torch.bfloat16)
            mean = torch.randn(C, device="cuda") * 0.1
            invstd = torch.rand(C, device="cuda") + 0.5
            gamma = torch.randn(C, device="cuda")
            sc, sh = gamma * invstd, -mean * gamma * invstd
            dy = torch.empty_like(y)
            dres = torch.empty_like(y) if res else None
            dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
            us = time_us(lambda: ops.bn_bwd(dout, y, out, relu, mean, invstd, gamma, M, C, dy,
                                            dres, dg, db, scale=sc, shift=sh), iters, 3, sync=False)
            tot += us
            print(f"bn_bwd M={M} C={C} relu={relu} res={res}: {us:.1f} us, "
                  f"{nbytes(M, C, relu, res) / us / 1e3:.0f} GB/s")
        print(f"total {tot:.1f} us  lib={lib_tag()}")
    return [(f"M={M} C={C} relu={relu} res={res}", nbytes(M, C, relu, res))
            for M, C, relu, res in shapes], run


@case(50, "B")
def colsum(B):
    """The bias-gradient column sum (dfu_colsum: partial sums + reduce) at the ViT shapes.
    Bytes: the bf16 dY read once (2 per element)."""
    rows = B * 197
    widths = sorted({N for _, N, _ in VIT_SHAPES.values()})

    def run(iters, tag):
        tot = 0.0
        for N in widths:
            x = _bf(rows, N)
            out = torch.zeros(N, device="cuda")
            us = time_us(lambda: ops.colsum_add(x, out), iters, 3, sync=False)
            tot += us
            print(f"colsum rows={rows} N={N}: {us:.1f} us, {rows * N * 2 / us / 1e3:.0f} GB/s")
        print(f"total {tot:.1f} us  lib={lib_tag()}")
    return [(f"rows={rows} N={N}", rows * N * 2) for N in widths], run


@case(50, "B")
def ln_fwd(B):
    """The ViT LayerNorm forward (fp32 residual stream in, bf16 out + mean/rstd).  Bytes per
    row: 4 D in + 2 D out.  Seeded inputs and an output checksum."""
    rows, D = B * 197, 768

    def run(iters, tag):
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.randn(rows, D, generator=g).cuda()
        gamma = torch.randn(D, generator=g).cuda()
        beta = torch.randn(D, generator=g).cuda()
        out = torch.empty(rows, D, dtype=torch.bfloat16, device="cuda")
        mean, rstd = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
        us = time_us(lambda: ops.layernorm_fwd(x, D, rows, D, gamma, beta, 1e-6, out, D, True,
                                               mean, rstd), iters, 3, sync=False)
        ck = (out.view(torch.int16).long().sum().item(), mean.double().sum().item(),
              rstd.double().sum().item())
        print(f"ln_fwd rows={rows} D={D} lib={lib_tag()}: {us:.1f} us, "
              f"{6 * D * rows / us / 1e3:.0f} GB/s algorithmic; checksum {ck}")
    return [(f"rows={rows} D={D}", 6 * D * rows)], run


@case(50, "B")
def ln_bwd(B):
    """The ViT LayerNorm backward (dfu_layernorm_bwd + dgamma/dbeta reduction): dy bf16, gx fp32
    read-modify-write + bf16 copy, column sums of gx.  Bytes per row: x 4D + gx 8D + dy 2D +
    gx_bf16 2D = 16 D."""
    rows, D = B * 197, 768

    def run(iters, tag):
        x = torch.randn(rows, D, device="cuda")
        dy = _bf(rows, D)
        gx = torch.randn(rows, D, device="cuda")
        gxb = torch.empty(rows, D, dtype=torch.bfloat16, device="cuda")
        mean = x.mean(1)
        rstd = torch.rsqrt(x.var(1, unbiased=False) + 1e-6)
        gamma = torch.randn(D, device="cuda")
        dg, db = torch.empty(D, device="cuda"), torch.empty(D, device="cuda")
        us = time_us(lambda: ops.layernorm_bwd(dy, D, True, x, D, mean, rstd, gamma, rows, D, gx,
                                               D, gxb, dg, db, gsum=True), iters, 3, sync=False)
        print(f"ln_bwd rows={rows} D={D} lib={lib_tag()}: {us:.1f} us, "
              f"{16 * D * rows / us / 1e3:.0f} GB/s algorithmic")
    return [(f"rows={rows} D={D}", 16 * D * rows)], run


@case(50, "B")
def pool(B):
    """The stem's max-pool backward (dfu_maxpool_bwd): dy [B][56][56][64] bf16 -> dx
    [B][112][112][64].  Bytes: dx written (2) + per pooled element dy (2) and the argmax (1)."""
    H, W, C = 112, 112, 64
    P, Q = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    nbytes = B * H * W * C * 2 + B * P * Q * C * 3

    def run(iters, tag):
        x = _bf(B * H * W, C)
        y, am, p, q = ops.maxpool_fwd(x, B, H, W, C)
        dy = _bf(B * p * q, C)
        dx = [None]  # the last result stays alive while the next is allocated

        def bwd():
            dx[0] = ops.maxpool_bwd(dy, am, B, H, W, C, p, q)
        us = time_us(bwd, iters, 1)
        print(f"maxpool bwd {B}x{H}x{W}x{C}: {us:.1f} us, {nbytes / us / 1e6:.2f} TB/s algorithmic")
    return [(f"{B}x{H}x{W}x{C}", nbytes)], run


@case(20, "FLOP")
def stem(B):
    """The parity mode's stem conv: the fused implicit-GEMM kernel (dfu_stem_conv_x3) against
    the pair im2col + split weights + interleaved-pair GEMM it replaces; and its weight gradient
    from x (dfu_stem_wgrad_x3) against the MN x MN GEMM over the hi im2col rows.  FLOPs: the
    7x7x3 conv's 2 M 64 147, forward or weight gradient."""
    M = B * 112 * 112

    def run(iters, tag):
        x = torch.randn(B, 3, 224, 224, device="cuda")
        w = torch.randn(64, 3, 7, 7, device="cuda") * 0.05

        def old():
            (chi, clo), P, Q = ops.im2col_f32_x3(x, 7, 7, 2, 3, 160)
            w3 = ops.split_x3(w.reshape(64, -1), ops.X3_PAIRS, seg=160)
            y = torch.empty(M, 64, dtype=torch.bfloat16, device="cuda")
            ylo = torch.empty_like(y)
            st = torch.empty(M // 128, 2, 64, device="cuda")
            ops.gemm(M, 64, 320, chi, 160, w3, 320, y, 64, epilogue=L.EPI_F32_STATS, stats=st,
                     x3=True, a_lo=clo, x3_pairs=True, aux_out=ylo, ldaux_out=64)
        dy = _bf(M, 64, scale=0.1)
        col = ops.im2col_f32(x, 7, 7, 2, 3, 160)[0]
        dw = torch.zeros(64, 147, device="cuda")

        def wgrad_gemm():
            ops.gemm(64, 147, M, dy, 64, col, 160, dw, 147, a_mode=L.OPND_MNMAJOR,
                     b_mode=L.OPND_MNMAJOR, epilogue=L.EPI_F32_ACC)
        for name, fn in (("pair im2col + GEMM", old),
                         ("fused stem kernel", lambda: ops.stem_conv_x3(x, w)),
                         ("fused, no col rows", lambda: ops.stem_conv_x3(x, w, want_col=False)),
                         ("wgrad: GEMM over col", wgrad_gemm),
                         ("wgrad: from x", lambda: ops.stem_wgrad_x3(x, dy, dw))):
            print(f"{name:20s}: {time_us(fn, iters, 3):8.1f} us per stem (B = {B})", flush=True)
    return [(f"{M}x64x147", 2 * M * 64 * 147)], run


@case(20, "FLOP")
def t1x1(B):
    """Layer 1's N = 64 1x1 input gradients (dX[M][64] = dY[M][K] W[K][64]): the MN-major weight
    view against the transposed [64][K] weight on each tile that runs it, with the result's
    relative error.  FLOPs: 2 M 64 K."""
    M = B * 56 * 56
    shapes = ((64, False), (256, False), (256, True))
    names = {0: "auto", 6: "128x128w4", 10: "256x64", 11: "128x64o2"}

    def run(iters, tag):
        for K, add in shapes:
            dy = _bf(M, K, scale=0.1)
            W = _bf(K, 64, scale=0.1)  # [out][in]
            Wt = W.t().contiguous()
            aux = _bf(M, 64, scale=0.1) if add else None
            epi = L.EPI_BF16_ADD if add else L.EPI_BF16
            ref = dy.float() @ W.float() + (aux.float() if add else 0)
            out = torch.empty(M, 64, dtype=torch.bfloat16, device="cuda")

            def mn(tile):
                ops.gemm(M, 64, K, dy, K, W, 64, out, 64, b_mode=L.OPND_MNMAJOR, epilogue=epi,
                         aux=aux, ldaux=64 if add else 0, tile=tile)

            def km(tile):
                ops.gemm(M, 64, K, dy, K, Wt, K, out, 64, epilogue=epi, aux=aux,
                         ldaux=64 if add else 0, tile=tile)
            cells = []
            for name, fn, tiles in (("MN-major W", mn, (0, 6)), ("W^T", km, (0, 6, 10, 11))):
                for t in tiles:
                    try:
                        us = time_us(lambda: fn(t), iters, 1)
                    except L.DfuError:
                        cells.append(f"{name}/{names[t]} -")
                        continue
                    err = ((out.float() - ref).norm() / ref.norm()).item()
                    cells.append(f"{name}/{names[t]} {us:6.1f}us (rel {err:.1e})")
            print(f"{M}x64x{K}{' ADD' if add else ''}: " + "  ".join(cells), flush=True)
    return [(f"{M}x64x{K}{' ADD' if add else ''}", 2 * M * 64 * K) for K, add in shapes], run


@case(20, "FLOP")
def dgrad_strided(B):
    """The ResNet-50 strided 3x3 input gradients (layer2-4 block 0 conv2) under every tile hint
    (0 = the library plan), and the stride-1 GEMM of each stride phase alone.  FLOPs: 2 Mx C K
    / 4, a quarter of the taps being live per phase."""
    shapes = [(56, 128), (28, 256), (14, 512)]  # input H = W, channels (C = K)
    flops = lambda H, C: 2 * (B * H * H) * C * (9 * C) / 4  # noqa: E731

    def run(iters, tag):
        for H, C in shapes:
            g = ops.ConvGeom(B, H, H, C, C, 3, 3, 2, 1)
            dy = _bf(B * g.p * g.q, C, scale=0.1)
            w = _bf(C, 3, 3, C, scale=0.1)  # KRSC
            dx = torch.empty(B * H * H, C, device="cuda", dtype=torch.bfloat16)
            Mx, K = B * H * H, 9 * C
            line = []
            for t in range(0, 12):
                try:
                    us = time_us(lambda: ops.gemm(Mx, C, K, dy, 0, w, K, dx, C,
                                                  a_mode=L.OPND_CONV_DGRAD,
                                                  b_mode=L.OPND_CONV_DGRAD_W, epilogue=L.EPI_BF16,
                                                  conv=g, tile=t), iters, 3, sync=False)
                    line.append(f"t{t} {us:6.1f}")
                except RuntimeError:
                    line.append(f"t{t}     --")
            print(f"dgrad s2 {Mx}x{C}x{K} (H={H}, C={C}) [{flops(H, C) / 1e9:.1f} GFLOP]: "
                  + "  ".join(line), flush=True)
            # each stride phase as the dense stride-1 GEMM it is: M = B (H/2)^2, K = live taps x C
            Mp = B * (H // 2) * (H // 2)
            for taps in (4, 2, 1):
                A, Bw = _bf(Mp, taps * C, scale=0.1), _bf(C, taps * C, scale=0.1)
                Cc = torch.empty(Mp, C, device="cuda", dtype=torch.bfloat16)
                us = time_us(lambda: ops.gemm(Mp, C, taps * C, A, taps * C, Bw, taps * C, Cc, C,
                                              epilogue=L.EPI_BF16), iters, 3, sync=False)
                print(f"   dense phase GEMM {Mp}x{C}x{taps * C}: {us:6.1f} us "
                      f"({2 * Mp * C * taps * C / us / 1e6:.0f} TF/s)", flush=True)
    return [(f"{B * H * H}x{C}x{9 * C} (H={H}, C={C})", flops(H, C)) for H, C in shapes], run


@case(30, "FLOP")
def epi(B):
    """The fc1 GEMM (persistent 256x256 tile) with its epilogues: BF16 (one bf16 output),
    F16_DUAL (one fp16 output) and F16_GELU (fp16 + bf16 gelu and bf16 gelu').  Seeded operands
    and checksums of the F16_GELU outputs; --tag leads the lines.  FLOPs: 2 M N K."""
    M, N, K = B * 197, VIT_SHAPES["fc1"][1], VIT_SHAPES["fc1"][2]
    f = 2.0 * M * N * K

    def run(iters, tag):
        torch.manual_seed(0)  # the same operands in every process: checksums compare across builds
        A = (torch.randn(M, K, device="cuda") * 0.5).half()
        Bw = (torch.randn(N, K, device="cuda") * 0.05).half()
        bias = torch.randn(N, device="cuda") * 0.1
        C2 = torch.empty(M, 2 * N, dtype=torch.bfloat16, device="cuda")
        C = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        D = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        bf = torch.bfloat16

        def gelu():
            ops.gemm(M, N, K, A, K, Bw, K, C2, 2 * N, epilogue=L.EPI_F16_GELU, bias=bias,
                     aux_out=D, ldaux_out=N, tile=8, operand_type=1)
        res = {
            "BF16 (bf16 operands)": time_us(
                lambda: ops.gemm(M, N, K, A.view(bf), K, Bw.view(bf), K, C, N,
                                 epilogue=L.EPI_BF16, bias=bias, tile=8), iters, 1),
            "F16_DUAL": time_us(
                lambda: ops.gemm(M, N, K, A, K, Bw, K, C, N, epilogue=L.EPI_F16_DUAL, bias=bias,
                                 tile=8, operand_type=1), iters, 1),
            "F16_GELU": time_us(gelu, iters, 1)}
        print(tag, " ".join(f"{k}: {v:.1f} us ({f / v / 1e6:.0f} TF)" for k, v in res.items()))
        gelu()
        torch.cuda.synchronize()
        print(tag, "F16_GELU output checksums (fp16 gelu | bf16 gelu | bf16 gelu'):",
              int(C2[:, :N].contiguous().view(torch.int16).long().sum()),
              int(C2[:, N:].contiguous().view(torch.int16).long().sum()),
              int(D.view(torch.int16).long().sum()))
    return [(f"{M}x{N}x{K}", f)], run


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("cases", nargs="*", metavar="case", help=" ".join(CASES))
    ap.add_argument("--all", action="store_true", help="every case")
    ap.add_argument("--batch", type=int, default=64, help="the B factor of every shape")
    ap.add_argument("--iters", type=int, default=None, help="default: each case's own count")
    ap.add_argument("--tag", default="product", help="leads the epi case's lines")
    ap.add_argument("--list", action="store_true", help="print the case names")
    ap.add_argument("--plan", action="store_true",
                    help="print shapes and algorithmic bytes or FLOPs; no GPU needed")
    a = ap.parse_args(argv)
    if a.list:
        print("\n".join(CASES))
        return
    names = list(CASES) if a.all or (a.plan and not a.cases) else a.cases
    if not names:
        ap.error("name a case, or --all")
    for n in names:
        if n not in CASES:
            ap.error(f"unknown case {n}; cases: {' '.join(CASES)}")
    if not a.plan:
        _harness.require_gpu()
    for n in names:
        fn, iters, unit = CASES[n]
        plan, run = fn(a.batch)
        if a.plan:
            for shape, work in plan:
                print(f"{n} {shape}: {int(work)} {unit}")
            continue
        if len(names) > 1:
            print(f"== {n}", flush=True)
        run(a.iters or iters, a.tag)


if __name__ == "__main__":
    main()
