"""Scaled RoPE for the compressed KV cache (transformers' rope types linear, dynamic, yarn and llama3).

The cache holds PRE-RoPE keys and the kernels rotate the dequantised keys at the column's position, so a model with
scaled RoPE needs nothing but another frequency table in the kernels (include/kvq.h: struct kvq_rope) and the same
table in the torch rotation of the query, the prefill keys and the fp16 sink keys (attention.RotaryDynamic).

The tables are transformers' own: `ROPE_INIT_FUNCTIONS[rope_type](config, device)` gives 64 fp32 inverse frequencies
and an attention factor `af`; HF multiplies cos and sin by `af` in fp32 and rounds them to the activation dtype.  Here
the query carries `af` through those rows, and the kernels multiply the compressed keys' (cos, sin) by `af` once more
(what the keys' own scaled rows would give).

  * "default": no table -- the kernels keep evaluating theta_j = powf(rope_theta, -2j/128) on the device (the
    reference's rule, bit for bit).  RopeSpec.table() returns None.
  * "linear", "llama3", "yarn": one fixed table per device.
  * "dynamic" (NTK): the table of a call is the one for seq_len = max(last position of the call + 1,
    max_position_embeddings), formed as LlamaRotaryEmbedding's dynamic update forms it (seq_len as a tensor).  Every cached key is rotated with the CURRENT table (the cache is pre-RoPE), which is
    HF's no-cache forward over the whole sequence -- not HF's cached generation, which keeps keys rotated with the
    tables of earlier steps.  The fp16 sink keys are stored post-RoPE, so dynamic scaling with sinks is refused.
  * "longrope", "proportional", other types and partial_rotary_factor != 1 raise ValueError.
"""
import math

import torch

SUPPORTED = ("default", "linear", "llama3", "yarn", "dynamic")
HEAD_DIM = 128


def _params_of(config):
    """(rope_type, parameter dict incl. rope_theta) of a transformers config: 5.x `rope_parameters`, 4.x `rope_scaling`
    + `rope_theta`, or neither (default RoPE)"""
    rp = getattr(config, "rope_parameters", None)
    if isinstance(rp, dict) and rp and "rope_theta" in rp and not any(isinstance(v, dict) for v in rp.values()):
        params = dict(rp)
    else:
        params = dict(getattr(config, "rope_scaling", None) or {})
        theta = getattr(config, "rope_theta", None)
        if theta is None and isinstance(rp, dict):
            theta = rp.get("rope_theta")
        params.setdefault("rope_theta", 10000.0 if theta is None else theta)
    rope_type = params.get("rope_type", params.get("type", "default")) or "default"
    params["rope_type"] = rope_type
    params.pop("type", None)
    return rope_type, params


class RopeSpec:
    """The RoPE of a layer: rope type, parameters (rope_theta, factor, ...), max_position_embeddings.  Built with
    RopeSpec.from_config(config) or RopeSpec.make(rope_theta, rope_scaling, max_position_embeddings); table(device,
    seq_len) gives the (inv_freq f32 [64] on `device`, attention factor) the kernels rotate with (None for default)."""

    def __init__(self, rope_type, params, max_position_embeddings=None):
        rope_type = rope_type or "default"
        if rope_type not in SUPPORTED:
            raise ValueError("scaled RoPE: rope_type %r is not supported (supported: %s)" % (rope_type, ", ".join(SUPPORTED)))
        prf = params.get("partial_rotary_factor", 1.0)
        if prf is not None and float(prf) != 1.0:
            raise ValueError("scaled RoPE (%s): partial_rotary_factor = %s is not supported (the kernels rotate all 128 "
                             "channels)" % (rope_type, prf))
        if rope_type != "default" and "factor" not in params:
            raise ValueError("scaled RoPE (%s): the parameters carry no 'factor'" % rope_type)
        if rope_type == "dynamic" and not max_position_embeddings:
            raise ValueError("scaled RoPE (dynamic): max_position_embeddings is required")
        self.rope_type = rope_type
        self.params = dict(params, rope_type=rope_type)
        self.rope_theta = float(self.params.get("rope_theta", 10000.0))
        self.max_position_embeddings = None if max_position_embeddings is None else int(max_position_embeddings)
        self._config = None
        self._tables = {}      # (device, seq_len or None) -> (inv_freq, af)

    @classmethod
    def from_config(cls, config):
        rope_type, params = _params_of(config)
        spec = cls(rope_type, params, getattr(config, "max_position_embeddings", None))
        if hasattr(config, "standardize_rope_params") and getattr(config, "head_dim", HEAD_DIM) == HEAD_DIM:
            spec._config = config     # (transformers' functions then read the model's own config)
        return spec

    @classmethod
    def make(cls, rope_theta=10000.0, rope_scaling=None, max_position_embeddings=None):
        """explicit arguments: rope_scaling is a 4.x `rope_scaling` / 5.x `rope_parameters` dict (or None, or a RopeSpec)"""
        if isinstance(rope_scaling, RopeSpec):
            return rope_scaling
        params = dict(rope_scaling or {})
        params.setdefault("rope_theta", rope_theta)
        rope_type = params.pop("type", None) or params.get("rope_type", "default")
        return cls(rope_type, params, max_position_embeddings)

    @property
    def is_default(self):
        return self.rope_type == "default"

    @property
    def dynamic(self):
        return self.rope_type == "dynamic"

    def hf_config(self):
        """a LlamaConfig with these parameters: what transformers' rope functions read (head_dim 128)"""
        if self._config is None:
            from transformers import LlamaConfig
            mpe = self.max_position_embeddings
            if mpe is None and "original_max_position_embeddings" in self.params:
                # (no model length given: the one the scaling implies, so that transformers' consistency checks hold)
                mpe = int(self.params["original_max_position_embeddings"] * float(self.params.get("factor", 1.0)))
            kw = {} if mpe is None else dict(max_position_embeddings=mpe)
            self._config = LlamaConfig(hidden_size=HEAD_DIM, num_attention_heads=1, num_key_value_heads=1,
                                       head_dim=HEAD_DIM, rope_parameters=dict(self.params), **kw)
        return self._config

    def table(self, device=None, seq_len=None):
        """(inv_freq f32 [64] on `device`, attention factor) -- bit for bit transformers' ROPE_INIT_FUNCTIONS -- or
        None for default RoPE.  Fixed types compute the table once (on the CPU, as a model built on the CPU and moved
        does) and keep one copy per device; dynamic computes it on `device` for seq_len = max(seq_len,
        max_position_embeddings) and keeps it per (device, seq_len), so that the layers of one token share it."""
        if self.is_default:
            return None
        dev = torch.device("cpu") if device is None else torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
        if self.dynamic:
            n = max(int(seq_len if seq_len is not None else 0), self.max_position_embeddings)
            key = (dev, n)
            hit = self._tables.get(key)
            if hit is None:
                # (as LlamaRotaryEmbedding's dynamic update: the table of max_position_embeddings up to it, beyond it the
                #  one for seq_len = max(position) + 1 passed as a tensor -- its arithmetic then runs in fp32 on `dev`)
                ln = None if n <= self.max_position_embeddings else torch.tensor(n, dtype=torch.int64, device=dev)
                inv, af = ROPE_INIT_FUNCTIONS["dynamic"](self.hf_config(), dev, seq_len=ln)
                hit = (self._check(inv.to(device=dev, dtype=torch.float32).contiguous()), float(af))
                # (a decode step asks for the next length: older lengths of this device are not asked for again)
                for k in [k for k in self._tables if k[0] == dev]:
                    del self._tables[k]
                self._tables[key] = hit
            return hit
        key = (dev, None)
        hit = self._tables.get(key)
        if hit is None:
            cpu = self._tables.get((torch.device("cpu"), None))
            if cpu is None:
                inv, af = ROPE_INIT_FUNCTIONS[self.rope_type](self.hf_config(), None)
                cpu = (self._check(inv.to(torch.float32).contiguous()), float(af))
                self._tables[(torch.device("cpu"), None)] = cpu
            hit = cpu if dev.type == "cpu" else (cpu[0].to(dev), cpu[1])
            self._tables[key] = hit
        return hit

    def pin_table(self, inv_freq, attention_factor):
        """use this table (a model's own rotary_emb.inv_freq / attention_scaling) for a fixed scaled type"""
        if self.is_default or self.dynamic:
            raise ValueError("scaled RoPE (%s): only the fixed types take a pinned table" % self.rope_type)
        inv = self._check(inv_freq.detach().to(device="cpu", dtype=torch.float32).contiguous())
        self._tables = {(torch.device("cpu"), None): (inv, check_factor(attention_factor))}

    def _check(self, inv):
        if tuple(inv.shape) != (HEAD_DIM // 2,):
            raise ValueError("scaled RoPE (%s): %d frequencies, the kernels take %d" % (self.rope_type, inv.numel(),
                                                                                     HEAD_DIM // 2))
        if not bool(torch.isfinite(inv).all()) or not bool((inv > 0).all()):
            raise ValueError("scaled RoPE (%s): the frequencies must be finite and > 0" % self.rope_type)
        return inv

    def __repr__(self):
        return "RopeSpec(%s, %r)" % (self.rope_type, {k: v for k, v in self.params.items() if k != "rope_type"})


def spec_of(rope_theta=10000.0, rope_scaling=None, max_position_embeddings=None):
    """RopeSpec from the arguments of KVQuantAttention / QuantK (rope_scaling: None, a dict or a RopeSpec)"""
    return RopeSpec.make(rope_theta, rope_scaling, max_position_embeddings)


def check_factor(af):
    af = float(af)
    if not (math.isfinite(af) and af > 0):
        raise ValueError("scaled RoPE: attention factor %r must be finite and > 0" % af)
    return af


def require_default(spec, route):
    """raise ValueError if `spec` is a scaled RoPE: `route` does not take a frequency table"""
    if spec is not None and not spec.is_default:
        raise ValueError("%s does not support scaled RoPE (rope_type %r): it rotates with the theta rule only"
                         % (route, spec.rope_type))
