"""ctypes binding of include/ddpo_optim.h: the Adafactor update of libddpo_hip.so, versioned on its own beside lib.py (ABI_VERSION here is
ddpo_optim_abi_version(), not lib.ABI_VERSION), and the host-side plan the kernels are driven by.

optax 0.1.5 `adafactor(learning_rate, weight_decay_rate)` keeps, for a tensor whose two largest axes are both >= min_dim_size_to_factor, the
means of g^2 + eps over each of those two axes instead of a full second moment.  In every U-Net inventory those two axes are
the last two, so such a tensor is S slabs of an R x C row-major matrix; `AdafactorPlan` refuses anything else.
"""
import ctypes
import math
from ctypes import c_double, c_int, c_int32, c_int64, c_size_t, c_void_p

import numpy as np
import torch

from . import lib as L

ABI_VERSION = 1          # must equal ddpo_optim_abi_version() of the loaded library (include/ddpo_optim.h)
TILE_ROWS = 128          # DDPO_ADAFACTOR_TILE_ROWS
CHUNK = 4096             # DDPO_ADAFACTOR_CHUNK

# optax.adafactor defaults the reference leaves alone
DECAY_RATE = 0.8
EPS = 1e-30
CLIPPING_THRESHOLD = 1.0
MIN_SCALE = 1e-3
MIN_DIM_SIZE_TO_FACTOR = 128


class AdafactorTensor(ctypes.Structure):
    """Mirror of ddpo_adafactor_tensor."""
    _fields_ = [("off", c_int64), ("numel", c_int64), ("v_off", c_int64), ("vc_off", c_int64), ("ws_off", c_int64),
                ("S", c_int32), ("R", c_int32), ("C", c_int32), ("factored", c_int32), ("norm_rows", c_int32),
                ("first_tile", c_int32), ("n_tiles", c_int32), ("reserved", c_int32)]


_SIGS = {
    "ddpo_optim_abi_version": (c_int, []),
    "ddpo_sizeof_adafactor_tensor": (c_size_t, []),
    "ddpo_adafactor_workspace_bytes": (c_size_t, [c_void_p, c_int, c_void_p, c_int, c_int, c_int64, c_int64]),
    "ddpo_adafactor_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int64, c_void_p,
                                    c_double, c_double, c_double, c_double, c_double, c_double, c_double, c_double, c_int,
                                    c_void_p, c_size_t, c_void_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGS)
_lib = None


def load():
    """Bind the optimizer entry points of libddpo_hip.so (idempotent).  A library without them is an error: there is no other path."""
    global _lib
    if _lib is None:
        lib = L.bind_side(_SIGS, "ddpo_optim_abi_version", ABI_VERSION, "optimizer", "lib_optim.py")
        if lib.ddpo_sizeof_adafactor_tensor() != ctypes.sizeof(AdafactorTensor):
            raise L.DdpoHipError("struct layout mismatch between include/ddpo_optim.h and ddpo_amd/lib_optim.py")
        _lib = lib
    return _lib


def factored_dims(shape, min_dim_size_to_factor=MIN_DIM_SIZE_TO_FACTOR):
    """optax `_factored_dims`: None, or (d1, d0) = the axes of the second-largest and the largest dimension (stable argsort)."""
    if len(shape) < 2:
        return None
    order = np.argsort(np.asarray(shape), kind="stable")
    if shape[order[-2]] < min_dim_size_to_factor:
        return None
    return int(order[-2]), int(order[-1])


def beta_t(count):
    """optax `_decay_rate_pow(count, 0.8)` in float32: 1 - (count + 1)^(-0.8); 0 on the first update."""
    return float(np.float32(1) - np.float32(count + 1) ** np.float32(-DECAY_RATE))


class AdafactorPlan:
    """Tensor table, work list and state layout for one flat buffer.  `shapes` / `offsets`: name -> shape / first element, in buffer order
    (a ParamStore's).  State layout, tensor after tensor: unfactored numel floats; factored S*R row statistics then S*C column statistics.
    Host-only until `.to(device)`; `entries` keeps (name, shape, AdafactorTensor) for whoever needs to read the state by name."""

    def __init__(self, shapes, offsets, numel, min_dim_size_to_factor=MIN_DIM_SIZE_TO_FACTOR):
        names = list(shapes)
        self.numel = int(numel)
        self.min_dim_size_to_factor = int(min_dim_size_to_factor)
        self.tensors = (AdafactorTensor * len(names))()
        self.entries = []
        work, slabs = [], []
        v_off = ws_off = tile = 0
        for i, name in enumerate(names):
            shape = tuple(int(s) for s in shapes[name])
            n = math.prod(shape)
            t = self.tensors[i]
            t.off, t.numel, t.first_tile = int(offsets[name]), n, tile
            fd = factored_dims(shape, min_dim_size_to_factor)
            if fd is None:
                t.S, t.R, t.C, t.factored, t.norm_rows = 1, 1, n, 0, 0
                t.v_off, t.n_tiles = v_off, (n + CHUNK - 1) // CHUNK
                v_off += n
            else:
                if set(fd) != {len(shape) - 2, len(shape) - 1}:
                    raise ValueError(f"{name}: shape {shape} factors over axes {fd}, not its last two: the kernels keep row / column "
                                     f"statistics of contiguous R x C slabs only")
                R, C = shape[-2], shape[-1]
                S = n // (R * C)
                ntr = (R + TILE_ROWS - 1) // TILE_ROWS
                t.S, t.R, t.C, t.factored, t.norm_rows = S, R, C, 1, int(fd[1] == len(shape) - 1)
                t.v_off, t.vc_off, t.ws_off, t.n_tiles = v_off, v_off + S * R, ws_off, S * ntr
                v_off += S * (R + C)
                ws_off += (S * (2 * R + C * (ntr + 1)) + 3) // 4 * 4
                slabs += [(i, s) for s in range(S)]
            work += [(i, k) for k in range(t.n_tiles)]
            tile += t.n_tiles
            self.entries.append((name, shape, t))
        self.n_state, self.n_tiles, self.n_slabs = v_off, tile, len(slabs)
        self.n_factored = sum(1 for _, _, t in self.entries if t.factored)
        # largest work items first: blocks are dispatched in list order, and a 5 MB tile that starts last would finish alone
        def elements(item):
            t = self.tensors[item[0]]
            return min(TILE_ROWS, t.R - (item[1] % -(-t.R // TILE_ROWS)) * TILE_ROWS) * t.C if t.factored else min(CHUNK, t.numel - item[1] * CHUNK)
        work.sort(key=elements, reverse=True)                   # stable: equal sizes keep table order
        self.work = np.asarray(work + slabs, dtype=np.int32).reshape(-1, 2)
        self.device = None

    @classmethod
    def for_store(cls, store, min_dim_size_to_factor=MIN_DIM_SIZE_TO_FACTOR):
        return cls(store.shapes, store.offsets, store.flat.numel(), min_dim_size_to_factor)

    def workspace_bytes(self):
        nb = load().ddpo_adafactor_workspace_bytes(ctypes.addressof(self.tensors), len(self.tensors), self.work.ctypes.data, self.n_tiles,
                                                   self.n_slabs, self.numel, self.n_state)
        if nb == 0:
            raise L.DdpoHipError("ddpo_adafactor_workspace_bytes rejected the plan")
        return int(nb)

    def to(self, device):
        """Upload the validated table and work list and allocate the workspace — once, when the optimizer state is created."""
        nb = self.workspace_bytes()
        raw = np.frombuffer(self.tensors, dtype=np.uint8).copy()
        self.d_tensors = torch.from_numpy(raw).to(device)
        self.d_work = torch.from_numpy(self.work.copy()).to(device)
        self.workspace = torch.zeros((nb + 7) // 8, dtype=torch.float64, device=device)
        self.workspace_nbytes = nb
        self.device = self.d_tensors.device
        return self

    def new_state(self):
        return torch.zeros(self.n_state, dtype=torch.float32, device=self.device)


def adafactor_step(p, g, state, plan, sqnorm, inv_n_acc, lr, count, weight_decay, max_grad_norm, eps=EPS,
                   clipping_threshold=CLIPPING_THRESHOLD, min_scale=MIN_SCALE, zero_grad=True):
    """One update in place (five launches on the current stream).  `count`: updates already applied.  `sqnorm`: the device double of lib.grad_sqnorm."""
    if plan.device is None:
        raise L.DdpoHipError("AdafactorPlan.to(device) has not been called")
    for name, t in (("p", p), ("g", g), ("state", state)):
        L._f32(t, name)
    if sqnorm.dtype != torch.float64 or not sqnorm.is_cuda:
        raise L.DdpoHipError(f"sqnorm must be a float64 CUDA tensor, got {sqnorm.dtype} on {sqnorm.device}")
    if p.numel() != plan.numel or g.numel() != plan.numel or state.numel() != plan.n_state:
        raise L.DdpoHipError(f"buffers of {p.numel()} / {g.numel()} / {state.numel()} elements against a plan for {plan.numel} / {plan.n_state}")
    if any(t.device != plan.device for t in (p, g, state, sqnorm)):
        raise L.DdpoHipError(f"the plan lives on {plan.device}")
    L._check(load().ddpo_adafactor_step(L._p(p), L._p(g), L._p(state), L._p(plan.d_tensors), len(plan.tensors), L._p(plan.d_work),
                                        plan.n_tiles, plan.n_slabs, plan.numel, L._p(sqnorm), float(inv_n_acc), float(lr),
                                        beta_t(count), float(eps), float(clipping_threshold), float(min_scale), float(weight_decay),
                                        float(max_grad_norm), int(zero_grad), L._p(plan.workspace), plan.workspace_nbytes, L._stream()),
             "ddpo_adafactor_step")
