"""The LoRA merge as the tests define it, and the inputs they feed it.

merge() is the reference: (W.float() + scale * (B.float() @ A.float())).to(torch.bfloat16) in torch on the CPU; merge64() evaluates the
same expression in fp64 without the final rounding.

Exact probes: base values are multiples of 2^-6 in [-2, 2], A and B integers in [-3, 3], the scale 2^-4.  Every partial sum of
B @ A is an integer of magnitude <= 9 * 256, scale times it a multiple of 2^-4 below 2^8, and adding a base value gives a multiple of
2^-6 below 2^9: fewer than 24 significant bits, so fp32 holds every intermediate exactly in ANY summation order and the only
rounding is the final one to bf16.  A kernel must therefore match merge() bit for bit.

General values: normal weights at std 0.02, A and B at std 0.1; bound() is the element-wise bound against the fp64 value y,
    |out - y| <= 0.5 ulp_bf16(y) + (r + 2) 2^-24 (|W| + |s| sum_j |B||A|),
half a bf16 ulp for the final rounding plus the fp32 accumulation bound of r products, the scaling and the base addition."""
from __future__ import annotations

import torch

PROBE_SCALE = 2.0 ** -4


def merge(W, A, B, scale):
    return (W.float() + scale * (B.float() @ A.float())).to(torch.bfloat16)


def merge64(W, A, B, scale):
    return W.double() + float(scale) * (B.double() @ A.double())


def merge_state_dict(sd, adapter, scale):
    """sd: HF name -> tensor; adapter: module path (the name without '.weight') -> (A, B).  The merged state dict: the base is what
    the engine holds of it (a checkpoint tensor rounded to bf16, as loading does), the factors likewise."""
    out = dict(sd)
    for mod, (A, B) in adapter.items():
        out[mod + ".weight"] = merge(sd[mod + ".weight"].to(torch.bfloat16), A.to(torch.bfloat16), B.to(torch.bfloat16), scale)
    return out


def probe_base(N, K, seed, ld=None):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randint(-128, 129, (N, ld or K), generator=g).float() / 64.0).to(torch.bfloat16)
    return w


def probe_ab(N, K, r, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed + 1000)
    A = torch.randint(-3, 4, (r, K), generator=g).to(dtype)
    B = torch.randint(-3, 4, (N, r), generator=g).to(dtype)
    return A, B


def general(N, K, r, seed):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn((N, K), generator=g) * 0.02).to(torch.bfloat16)
    A = (torch.randn((r, K), generator=g) * 0.1).to(torch.bfloat16)
    B = (torch.randn((N, r), generator=g) * 0.1).to(torch.bfloat16)
    return W, A, B


def ulp_bf16(y):
    """Spacing of bf16 around |y| (fp64 in, fp64 out): 2^(floor(log2 |y|) - 7), the smallest normal's spacing below it."""
    e = torch.floor(torch.log2(y.abs().clamp(min=2.0 ** -126)))
    return torch.exp2(e - 7)


def bound(W, A, B, scale):
    y = merge64(W, A, B, scale)
    mag = W.double().abs() + abs(float(scale)) * (B.double().abs() @ A.double().abs())
    return y, 0.5 * ulp_bf16(y) + (A.shape[0] + 2) * 2.0 ** -24 * mag


def peft_names(adapter, prefix="base_model.model.", adapter_name=None):
    """module path -> (A, B)  =>  peft's (name, tensor) pairs."""
    mid = "" if adapter_name is None else "." + adapter_name
    out = []
    for mod, (A, B) in adapter.items():
        out.append((f"{prefix}{mod}.lora_A{mid}.weight", A))
        out.append((f"{prefix}{mod}.lora_B{mid}.weight", B))
    return out


LLM_LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
               "mlp.down_proj")


def probe_adapter(sd, modules, r, seed=0, dtype=torch.bfloat16, zero_b=False):
    """An exact-probe adapter (A, B integers in [-3, 3]) on the named modules of state dict `sd`."""
    out = {}
    for i, mod in enumerate(modules):
        N, K = sd[mod + ".weight"].shape
        A, B = probe_ab(N, K, r, seed + i, dtype)
        out[mod] = (A, torch.zeros_like(B) if zero_b else B)
    return out
