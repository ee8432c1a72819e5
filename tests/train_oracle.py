"""The CPU-oracle yardstick of a whole amp-O2 HRNet-W32 training step (4 crops of 128x96), shared by
tests/test_gpu_train_full.py::test_o2_training_step_vs_oracle_amp_emulation and the switch matrix of
tests/test_gpu_train_switches.py: the eager HIP step, run under whatever switches the caller set, against oracle/nets.py
`net_forward_train` - once with the amp-O2 emulation (fp16 operands and cell outputs, fp32 accumulation / statistics), once in
fp32.  The two oracle runs depend on nothing a switch changes and are cached per process."""
import functools

import numpy as np
import torch

import mindpose_amd as mp
from oracle import nets as onets

DEV = torch.device("cuda:0")
SCALE = 1024.0


def data(n, h, w, seed=11):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, h, w, generator=g)
    kp = torch.empty(n, 17, 3)
    kp[..., 0] = torch.rand(n, 17, generator=g) * (w + 40) - 20
    kp[..., 1] = torch.rand(n, 17, generator=g) * (h + 40) - 20
    kp[..., 2] = (torch.rand(n, 17, generator=g) < 0.7).float()
    return x, kp


@functools.lru_cache(maxsize=None)
def _problem():
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "hrnet_head"), seed=0)
    cpu_state = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}  # before the network moves to the GPU
    names = [k for k, _ in net.named_parameters()]
    x, kp = data(4, 128, 96)
    tgt = mp.TopDownGenerateTarget(config=dict(image_size=[96, 128], heatmap_size=[24, 32]), sigma=2.0)
    target, weight = tgt(kp.to(DEV))
    return cpu_state, names, x, target, weight


def hip_step():
    """The eager amp-O2 step on the GPU under the CURRENT environment: (loss, {parameter name: flat fp64 gradient on the CPU})."""
    cpu_state, _, x, target, weight = _problem()
    net = mp.create_network("hrnet_w32", "hrnet_head")
    net.load_state_dict({k: v.clone() for k, v in cpu_state.items()})  # the very parameters the oracle runs hold
    net = net.to(DEV).train()
    mp.models.auto_mixed_precision(net, "O2")
    nwl = mp.create_network_with_loss(net, mp.create_loss("joint_mse", use_target_weight=True), has_extra_inputs=True)
    loss = nwl(x.to(DEV), target, weight)
    (loss * SCALE).backward()
    torch.cuda.synchronize()
    return float(loss.detach()), {k: (v.grad / SCALE).double().cpu().flatten() for k, v in net.named_parameters()}


@functools.lru_cache(maxsize=None)
def oracle(amp: bool):
    """(loss, gradients) of the oracle's training step; ``amp``: its amp-O2 emulation, else fp32."""
    cpu_state, names, x, target, weight = _problem()
    p = {k: v.clone() for k, v in cpu_state.items()}
    for k, v in p.items():
        if v.dtype.is_floating_point and not k.endswith(("moving_mean", "moving_variance")):
            v.requires_grad_()
    out = onets.net_forward_train(p, x, "hrnet_w32", "hrnet_head", amp=amp)
    l = (((out - target.cpu()) ** 2) * weight.cpu()[..., None, None]).mean()
    (l * SCALE).backward()
    return float(l.detach()), {k: (p[k].grad / SCALE).double().flatten() for k in names}


def cos(a, b):
    return float((a @ b) / (a.norm() * b.norm()).clamp_min(1e-300))


def check_against_oracle(loss: float, got, what: str = "O2 step") -> None:
    """The acceptance of the amp-O2 step: loss within 5e-3 of the emulation's; global cosine > 0.98, median per-tensor cosine > 0.99,
    minimum > 0.97 against the emulation; at most 1.5x (+ 1e-4) as far from the fp32 gradients as the emulation is; the layer next
    to the loss within 5e-3."""
    l_amp, g_amp = oracle(True)
    l_f32, g_f32 = oracle(False)
    assert abs(loss - l_amp) <= 5e-3 * abs(l_amp), (loss, l_amp, l_f32)
    c_amp = {k: cos(got[k], g_amp[k]) for k in got}          # HIP O2 vs the emulation
    c_hip_f32 = {k: cos(got[k], g_f32[k]) for k in got}      # HIP O2 vs fp32 truth
    c_emu_f32 = {k: cos(g_amp[k], g_f32[k]) for k in got}    # emulation vs fp32 truth
    all_hip, all_amp, all_f32 = (torch.cat([d[k] for k in got]) for d in (got, g_amp, g_f32))
    print(f"{what}: loss {loss:.6f} / emulation {l_amp:.6f} / fp32 {l_f32:.6f}; global cosine vs emulation "
          f"{cos(all_hip, all_amp):.5f}, vs fp32 {cos(all_hip, all_f32):.5f} (emulation vs fp32 {cos(all_amp, all_f32):.5f}); "
          f"per-tensor vs emulation median {np.median(list(c_amp.values())):.5f} min {min(c_amp.values()):.4f}")
    assert cos(all_hip, all_amp) > 0.98 and np.median(list(c_amp.values())) > 0.99 and min(c_amp.values()) > 0.9
    # per-tensor floor 0.97 (measured minimum 0.9736: BatchNorm parameters of the deepest layers, whose gradient is a
    # small difference of large sums - the emulation itself sits that far from the fp32 gradient on them)
    low = sorted((k for k in got if c_amp[k] < 0.98), key=lambda k: c_amp[k])
    for k in low[:8]:
        print(f"  lowest: {k} numel {got[k].numel()} cos(hip, emu) {c_amp[k]:.4f} cos(hip, f32) {c_hip_f32[k]:.4f} "
              f"cos(emu, f32) {c_emu_f32[k]:.4f}")
    assert min(c_amp.values()) > 0.97
    # distance to the fp32 gradients: not worse than the op-by-op emulation of the reference's recipe
    assert 1 - cos(all_hip, all_f32) <= 1.5 * (1 - cos(all_amp, all_f32)) + 1e-4
    assert np.median([1 - c for c in c_hip_f32.values()]) <= 1.5 * np.median([1 - c for c in c_emu_f32.values()]) + 1e-4
    # one layer from the loss: tight against the emulation
    for name in ("head.head.weight", "head.head.bias"):
        rel = float((got[name] - g_amp[name]).abs().max() / g_amp[name].abs().max())
        assert rel < 5e-3, (name, rel)
