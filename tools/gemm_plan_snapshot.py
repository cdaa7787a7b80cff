"""Record what the GEMM planner answers for a fixed set of descriptors (no GPU needed):
dfu_gemm_plan's return code, tile and split-K, dfu_gemm_workspace_bytes, and the workspace
bytes again with the tail split off.  tests/test_host_cpu.py replays tests/golden/gemm_plans.json
against the built library, so a change of the dispatch code that moves a plan shows up there.

The fixture is recorded from the commit BEFORE such a change, never from the code under test:
    DFU_HIP_LIB=<that build's libdfu_hip.so> python tools/gemm_plan_snapshot.py \
        > tests/golden/gemm_plans.json

Cases: every row of csrc/gemm_tuned.inc; its bf16 rows again with fp16 operands where no fp16
row exists (the fall-back to the bf16 plan, or "unsupported"); the convolutions of the training
step (forward, dgrad at stride 1 and 2 -- the latter the strided-dgrad workspace bound --, wgrad)
at B = 3 and 64; a fixed-seed sweep of untuned shapes over both linear operand modes, eleven
epilogues, tile hints 0..11, split_k 0 / 1 / fixed, M down to 1, N and K ragged against every
tile size; and small F32_ACC shapes on the automatic plan (M, N <= 2048, K <= 8192), the range
in which a schedule-dependent cost model would move the split-K."""
import ctypes
import json
import os
import random
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dfu-multimodal_amd")]
from dfu_hip import _lib as L  # noqa: E402

# a case: these descriptor fields (the conv geometry only on conv descriptors) ...
LINEAR = ["M", "N", "K", "a_mode", "b_mode", "epilogue", "split_k", "tile", "operand_type",
          "x3_pairs"]
CONV = ["conv_n", "conv_h", "conv_w", "conv_c", "conv_k", "conv_r", "conv_s", "conv_stride",
        "conv_pad"]
# ... followed by the recorded answers
RESULT = ["rc", "tile", "split_k", "workspace_bytes", "workspace_bytes_no_tail_split"]

SWEEP_EPIS = [L.EPI_BF16, L.EPI_BF16_RELU, L.EPI_BF16_GELU, L.EPI_F32, L.EPI_F32_RESID,
              L.EPI_BF16_DGELU, L.EPI_BF16_ADD, L.EPI_F32_ACC, L.EPI_BF16_STATS, L.EPI_PATCH,
              L.EPI_F32_STATS]
# F32_ACC shapes (MN-major A and B, automatic plan: tile 6, split-K 2) that the cost model
# split 5 ways under dfu_gemm_set_persistent(1) while it still priced the persistent schedule
SCHEDULE_SENSITIVE = [(1949, 1292, 8000), (1957, 1283, 7944)]
STEP_CONVS = [  # H, C, K, R, stride: the ResNet-50 convolutions of the step
    (56, 64, 64, 1, 1), (56, 64, 64, 3, 1), (56, 64, 256, 1, 1), (56, 256, 64, 1, 1),
    (56, 256, 128, 1, 1), (56, 128, 128, 3, 2), (28, 128, 512, 1, 1), (56, 256, 512, 1, 2),
    (28, 512, 128, 1, 1), (28, 128, 128, 3, 1), (28, 512, 256, 1, 1), (28, 256, 256, 3, 2),
    (14, 256, 1024, 1, 1), (28, 512, 1024, 1, 2), (14, 1024, 256, 1, 1), (14, 256, 256, 3, 1),
    (14, 1024, 512, 1, 1), (14, 512, 512, 3, 2), (7, 512, 2048, 1, 1), (14, 1024, 2048, 1, 2),
    (7, 2048, 512, 1, 1), (7, 512, 512, 3, 1)]


def make_desc(case):
    """The descriptor of a case (its LINEAR fields, then CONV if it has them)."""
    d = L.GemmDesc()
    for f, v in zip(LINEAR + CONV, case):
        setattr(d, f, v)
    if len(case) >= len(LINEAR) + len(CONV):
        d.conv_p = (d.conv_h + 2 * d.conv_pad - d.conv_r) // d.conv_stride + 1
        d.conv_q = (d.conv_w + 2 * d.conv_pad - d.conv_s) // d.conv_stride + 1
    d.lda = d.M if d.a_mode == L.OPND_MNMAJOR else d.K
    d.ldb = d.N if d.b_mode == L.OPND_MNMAJOR else d.K
    d.ldc = 3 * d.N  # (F16_GELU, X3_GELU: C holds two / three planes)
    d.alpha = 1.0
    if d.epilogue in (L.EPI_F16_GELU, L.EPI_X3_GELU):
        d.aux_out, d.ldaux_out = 1 << 20, d.N  # never dereferenced by the planner
    if d.x3_pairs:
        d.a_seg, d.a_lo = (d.conv_c if d.a_mode == L.OPND_CONV_FWD else d.K) // 2, 1 << 20
    return d


def answers(lib, case):
    """RESULT for a case from the loaded library."""
    d = make_desc(case)
    t, sk = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib.dfu_gemm_plan(ctypes.byref(d), ctypes.byref(t), ctypes.byref(sk))
    ws = lib.dfu_gemm_workspace_bytes(ctypes.byref(d))
    old = lib.dfu_gemm_set_tail_split(0)
    try:
        ws0 = lib.dfu_gemm_workspace_bytes(ctypes.byref(d))
    finally:
        lib.dfu_gemm_set_tail_split(old)
    return [rc, t.value, sk.value, ws, ws0]


def tuned_cases():
    rows = []
    with open(os.path.join(ROOT, "dfu-multimodal_amd", "csrc", "gemm_tuned.inc")) as f:
        for line in f:
            m = re.match(r"\s*\{([-\d,\s]+)\}", line)
            if m:
                rows.append([int(x) for x in m.group(1).split(",")])
    keys = {tuple(r[:15]) for r in rows}
    out = []
    for half in (0, 1):  # the rows themselves, then the fp16 fall-backs of the bf16 rows
        for a, b, e, M, N, K, *conv in (r[:15] for r in rows):
            if half and (e & 192 or (a, b, e | 64, M, N, K, *conv) in keys):
                continue
            case = [M, N, K, a, b, e & 63, 0, 0, 1 if half or e & 64 else 0, 1 if e & 128 else 0]
            out.append(case + (conv if a >= L.OPND_CONV_FWD or b >= L.OPND_CONV_FWD else []))
    return out


def conv_cases():
    out = []
    for B in (3, 64):
        for H, C, K, R, st in STEP_CONVS:
            pad = R // 2
            P = (H + 2 * pad - R) // st + 1
            geom = [B, H, H, C, K, R, R, st, pad]
            fwd_a = L.OPND_KMAJOR if R == 1 and st == 1 else L.OPND_CONV_FWD
            out.append([B * P * P, K, R * R * C, fwd_a, L.OPND_KMAJOR, L.EPI_BF16_STATS, 0, 0, 0, 0]
                       + geom)
            out.append([B * H * H, C, R * R * K, L.OPND_CONV_DGRAD, L.OPND_CONV_DGRAD_W,
                        L.EPI_BF16_ADD, 0, 0, 0, 0] + geom)
            out.append([K, R * R * C, B * P * P, L.OPND_MNMAJOR, L.OPND_CONV_WGRAD_X,
                        L.EPI_F32_ACC, 0, 0, 0, 0] + geom)
    return out


def sweep_cases():
    rnd = random.Random(1234)
    edges = [64, 128, 192, 256]  # every tile extent

    def ragged(hi):  # 1 .. hi, half of them next to a multiple of a tile extent
        if rnd.random() < 0.5:
            return rnd.randint(1, hi)
        e = rnd.choice(edges)
        return max(1, min(hi, e * rnd.randint(1, max(1, hi // e)) + rnd.choice([-8, -1, 0, 1, 8])))

    out = []
    for i in range(1200):
        M = ragged(rnd.choice([300, 5000, 300000]))
        N = ragged(4096)
        K = 8 * ragged(2048)
        e = SWEEP_EPIS[i % 11]
        tile = rnd.randint(1, 11) if rnd.random() < 0.4 else 0
        split = rnd.choice([0, 1, rnd.randint(2, 64)]) if e == L.EPI_F32_ACC else 0
        out.append([M, N, K, rnd.randint(0, 1), rnd.randint(0, 1), e, split, tile, 0, 0])
    for i in range(300):  # small weight gradients on the automatic plan
        out.append([ragged(2048), ragged(2048), 8 * ragged(1024), L.OPND_MNMAJOR, L.OPND_MNMAJOR,
                    L.EPI_F32_ACC, 0, 0, 0, 0])
    for M, N, K in SCHEDULE_SENSITIVE:
        out.append([M, N, K, L.OPND_MNMAJOR, L.OPND_MNMAJOR, L.EPI_F32_ACC, 0, 0, 0, 0])
    return out


def all_cases():
    return tuned_cases() + conv_cases() + sweep_cases()


if __name__ == "__main__":
    lib = L.load()
    cases = [c + answers(lib, c) for c in all_cases()]
    print(json.dumps({"linear": LINEAR, "conv": CONV, "result": RESULT}, separators=(",", ":"))[:-1]
          + ',"cases":[')
    print(",\n".join(json.dumps(c, separators=(",", ":")) for c in cases))
    print("]}")
