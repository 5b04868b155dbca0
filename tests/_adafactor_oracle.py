"""Oracle (test infrastructure only): optax 0.1.5 `adafactor(learning_rate, weight_decay_rate)` behind `clip_by_global_norm`, in numpy, in
float32 (what the kernels are held to) or float64 (what the float32 restatement's own error is measured against).

optax and jax are not installed: PARITY UNPINNED, as for oracle/optim.py.  Restated from optax 0.1.5:
  factorized.scale_by_factored_rms(factored=True, decay_rate=0.8, step_offset=0, min_dim_size_to_factor=128, epsilon=1e-30)
      decay = 1 - (count + 1)^(-0.8)                       (float32; 0 on the first update)
      g2 = g^2 + eps
      unfactored (len(shape) < 2 or second-largest dim < 128):   v = decay v + (1 - decay) g2 ;  u = g v^(-1/2)
      factored, d1 / d0 = axes of the second-largest / largest dim (stable argsort):
          v_row = decay v_row + (1 - decay) mean(g2, d0) ;  v_col = decay v_col + (1 - decay) mean(g2, d1)
          u = g * expand(  (v_row / mean(v_row, axis d1 as it sits in v_row, keepdims))^(-1/2), d0) * expand(v_col^(-1/2), d1)
  clipping.clip_by_block_rms(1.0):         u /= max(1, sqrt(mean(u^2)) / 1.0)
  scale by learning_rate (sign kept)
  transform.scale_by_param_block_rms():    u *= max(sqrt(mean(p^2)), 1e-3)
  transform.add_decayed_weights(wd):       u += wd p            (NOT multiplied by the learning rate)
  scale(-1):                               p <- p - u
Same interface as oracle.optim.AdamWBf16Mu, so oracle.optim.AccumulatingState drives it unchanged.
"""
import numpy as np

from oracle.optim import global_norm


def factored_dims(shape, min_dim_size_to_factor):
    if len(shape) < 2:
        return None
    order = np.argsort(shape, kind="stable")
    if shape[order[-2]] < min_dim_size_to_factor:
        return None
    return int(order[-2]), int(order[-1])


class Adafactor:
    def __init__(self, lr=1e-5, weight_decay=1e-4, max_grad_norm=1.0, min_dim_size_to_factor=128, decay_rate=0.8, eps=1e-30,
                 clipping_threshold=1.0, min_scale=1e-3, dtype=np.float32):
        self.lr, self.wd, self.max_norm, self.min_dim = lr, weight_decay, max_grad_norm, min_dim_size_to_factor
        self.decay_rate, self.eps, self.thr, self.min_scale, self.T = decay_rate, eps, clipping_threshold, min_scale, dtype
        self.trace = []         # per update: which branches were taken

    def init(self, params):
        T, v = self.T, []
        for p in params:
            fd = factored_dims(p.shape, self.min_dim)
            if fd is None:
                v.append({"v": np.zeros(p.shape, T)})
            else:
                d1, d0 = fd
                v.append({"v_row": np.zeros(np.delete(p.shape, d0), T), "v_col": np.zeros(np.delete(p.shape, d1), T)})
        return {"count": 0, "v": v}

    def update(self, params, grads, state):
        """One optimizer step; returns (new_params, new_state, grad_norm_before_clip)."""
        T = self.T
        if T is np.float32:
            gn = global_norm(grads)
        else:
            gn = np.sqrt(np.sum([np.sum(g.astype(np.float64) ** 2) for g in grads]))
        clipped = not (gn < T(self.max_norm))
        g_c = [g.astype(T) for g in grads] if not clipped else [((g.astype(T) / gn) * T(self.max_norm)).astype(T) for g in grads]
        decay = T(np.float32(1) - np.float32(state["count"] + 1) ** np.float32(-self.decay_rate))
        mix = T(1) - decay
        new_p, new_v, rms_clip, floor = [], [], [], []
        for p, g, s in zip(params, g_c, state["v"]):
            p = p.astype(T)
            g2 = g * g + T(self.eps)
            fd = factored_dims(p.shape, self.min_dim)
            if fd is None:
                v = decay * s["v"] + mix * g2
                u = g * (T(1) / np.sqrt(v))
                new_v.append({"v": v.astype(T)})
            else:
                d1, d0 = fd
                v_row = (decay * s["v_row"] + mix * np.mean(g2, axis=d0, dtype=T)).astype(T)
                v_col = (decay * s["v_col"] + mix * np.mean(g2, axis=d1, dtype=T)).astype(T)
                rd1 = d1 - 1 if d1 > d0 else d1
                m = np.mean(v_row, axis=rd1, keepdims=True, dtype=T)
                u = g * np.expand_dims(T(1) / np.sqrt(v_row / m), d0) * np.expand_dims(T(1) / np.sqrt(v_col), d1)
                new_v.append({"v_row": v_row, "v_col": v_col})
            rms_u = np.sqrt(np.mean(u * u, dtype=T))
            u = u / np.maximum(T(1), rms_u / T(self.thr))
            u = T(self.lr) * u
            rms_p = np.sqrt(np.mean(p * p, dtype=T))
            u = u * np.maximum(rms_p, T(self.min_scale))
            u = u + T(self.wd) * p
            new_p.append((p - u).astype(T))
            rms_clip.append(bool(rms_u > T(self.thr)))
            floor.append(bool(rms_p < T(self.min_scale)))
        self.trace.append({"global_clip": clipped, "block_rms_clip": rms_clip, "min_scale": floor, "grad_norm": float(gn)})
        return new_p, {"count": state["count"] + 1, "v": new_v}, gn


def state_from_flat(plan, flat):
    """The kernels' flat state buffer as the oracle's per-tensor dicts.  The plan keeps per slab R row statistics then C column statistics;
    optax's v_row is whichever of the two is left after reducing the LARGEST of the last two axes (norm_rows: the row statistics)."""
    out = []
    for name, shape, t in plan.entries:
        if not t.factored:
            out.append({"v": flat[t.v_off:t.v_off + t.numel].reshape(shape)})
            continue
        rows = flat[t.v_off:t.v_off + t.S * t.R].reshape(shape[:-2] + (t.R,))
        cols = flat[t.vc_off:t.vc_off + t.S * t.C].reshape(shape[:-2] + (t.C,))
        out.append({"v_row": rows, "v_col": cols} if t.norm_rows else {"v_row": cols, "v_col": rows})
    return out
