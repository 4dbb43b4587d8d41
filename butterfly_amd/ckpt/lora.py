"""LoRA adapter directories: butterfly-lora v1 and HuggingFace PEFT.

Both forms load into the same thing: logical tensors named like the base checkpoint's weights,
`layers.{i}.attn.{q,k,v,o}_proj.lora_A` [r, K] and `.lora_B` [N, r] (likewise
`mlp.{gate,up,down}_proj`), and one scale, which TransformerLM.load_lora places into a slot.

  butterfly-lora v1   adapter.json {"format": "butterfly-lora", "version": 1, "rank", "alpha",
                      "base_model"} + adapter.safetensors under the logical names; scale = alpha / rank
  PEFT                adapter_config.json {"r", "lora_alpha", "target_modules", "use_rslora"?} +
                      adapter_model.safetensors with keys ...layers.N.self_attn.{q,k,v,o}_proj.
                      lora_{A,B}.weight and ...mlp.{gate,up,down}_proj...; scale = lora_alpha / r,
                      or lora_alpha / sqrt(r) with use_rslora

A key that is none of the seven targets of a decoder layer (embeddings, LM head, other modules)
raises ValueError: dropping it would serve a different model than the one that was trained.
"""
from __future__ import annotations

import json
import math
import os
import re
from dataclasses import dataclass
from pathlib import Path

import torch
from safetensors import safe_open
from safetensors.torch import save_file

LORA_FORMAT = "butterfly-lora"
LORA_VERSION = 1

_LOGICAL = re.compile(r"layers\.\d+\.(attn\.(q|k|v|o)_proj|mlp\.(gate|up|down)_proj)\.lora_[AB]")
_PEFT = [
    (r"(?:.*\.)?layers\.(\d+)\.self_attn\.(q|k|v|o)_proj\.lora_(A|B)(?:\.\w+)?\.weight", r"layers.\1.attn.\2_proj.lora_\3"),
    (r"(?:.*\.)?layers\.(\d+)\.mlp\.(gate|up|down)_proj\.lora_(A|B)(?:\.\w+)?\.weight", r"layers.\1.mlp.\2_proj.lora_\3"),
]


@dataclass
class LoraAdapter:
    tensors: dict          # logical name -> tensor (lora_A [r, K], lora_B [N, r])
    rank: int
    alpha: float
    scale: float
    base_model: str = ""


def peft_name(key: str) -> str:
    """The logical name of a PEFT tensor key; ValueError for any other module."""
    for pat, rep in _PEFT:
        if re.fullmatch(pat, key):
            return re.sub(pat, rep, key)
    raise ValueError(f"LoRA adapter: unsupported tensor {key!r} (only the q / k / v / o / gate / up / down "
                     "projections of decoder layers can carry an adapter)")


def _read(path: Path) -> dict:
    with safe_open(str(path), framework="pt") as fh:
        return {k: fh.get_tensor(k) for k in fh.keys()}


def _check_ranks(tensors: dict, rank: int) -> None:
    for name, t in tensors.items():
        r = t.shape[0] if name.endswith("lora_A") else t.shape[-1]
        if t.dim() != 2 or r != rank:
            raise ValueError(f"LoRA adapter: {name} has shape {tuple(t.shape)}, the adapter's rank is {rank}")


def save_lora(path: str | os.PathLike, tensors: dict, rank: int, alpha: float, base_model: str = "") -> None:
    """Write a butterfly-lora v1 directory from logical tensors."""
    path = Path(path)
    for name in tensors:
        if not _LOGICAL.fullmatch(name):
            raise ValueError(f"LoRA adapter: unsupported tensor {name!r}")
    _check_ranks(tensors, int(rank))
    path.mkdir(parents=True, exist_ok=True)
    save_file({k: v.detach().cpu().contiguous() for k, v in tensors.items()}, str(path / "adapter.safetensors"))
    meta = {"format": LORA_FORMAT, "version": LORA_VERSION, "rank": int(rank), "alpha": float(alpha),
            "base_model": base_model}
    (path / "adapter.json").write_text(json.dumps(meta, indent=1))


def load_lora(path: str | os.PathLike) -> LoraAdapter:
    """Read an adapter directory of either form."""
    path = Path(path)
    if (path / "adapter.json").exists():
        meta = json.loads((path / "adapter.json").read_text())
        if meta.get("format") != LORA_FORMAT or meta.get("version") != LORA_VERSION:
            raise ValueError(f"LoRA adapter {path}: not a {LORA_FORMAT} v{LORA_VERSION} directory")
        tensors = _read(path / "adapter.safetensors")
        for name in tensors:
            if not _LOGICAL.fullmatch(name):
                raise ValueError(f"LoRA adapter {path}: unsupported tensor {name!r}")
        rank, alpha = int(meta["rank"]), float(meta["alpha"])
        _check_ranks(tensors, rank)
        return LoraAdapter(tensors, rank, alpha, alpha / rank, meta.get("base_model", ""))
    if (path / "adapter_config.json").exists():
        meta = json.loads((path / "adapter_config.json").read_text())
        if meta.get("peft_type", "LORA") != "LORA" or meta.get("use_dora"):
            raise ValueError(f"LoRA adapter {path}: only plain LoRA adapters are supported")
        tensors = {peft_name(k): v for k, v in _read(path / "adapter_model.safetensors").items()}
        rank, alpha = int(meta["r"]), float(meta["lora_alpha"])
        _check_ranks(tensors, rank)
        scale = alpha / math.sqrt(rank) if meta.get("use_rslora") else alpha / rank
        return LoraAdapter(tensors, rank, alpha, scale, meta.get("base_model_name_or_path") or "")
    raise FileNotFoundError(f"no adapter.json or adapter_config.json in {path}")
