"""Where the eager C3 step's runtime copies and fills come from (tools, not a product path): one
profiled step (torch.profiler, Python stacks), the ATen copy / fill / zero ops grouped by their
calling site in this repository.

  python tools/copy_sites.py
"""
import _harness
import torch

OPS = ("aten::copy_", "aten::clone", "aten::contiguous", "aten::to", "aten::_to_copy",
       "aten::fill_", "aten::zero_", "aten::zeros", "aten::zeros_like", "aten::cat",
       "aten::index", "aten::mul", "aten::add", "aten::sub", "aten::div")


def main():
    step = _harness.fusion_step().step
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    torch.autograd.set_multithreading_enabled(False)  # backward frames on this thread
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU], with_stack=True) as prof:
        step()
        torch.cuda.synchronize()
    sites = {}
    for ev in prof.events():
        if ev.name not in OPS:
            continue
        frames = [f for f in (ev.stack or []) if "dfu-multimodal_amd" in f or "bench.py" in f]
        key = (ev.name, frames[0] if frames else "(no repo frame)")
        sites[key] = sites.get(key, 0) + 1
    for (name, frame), n in sorted(sites.items(), key=lambda kv: -kv[1]):
        print(f"{n:4d}  {name:18s} {frame}")


if __name__ == "__main__":
    main()
