"""The optimizer step on the device: global-norm clip + AdamW over all parameter tensors of a model in three launches
(csrc/hgt_optim.hip) -- the line every script of the reference ends a step with,

    torch.nn.utils.clip_grad_norm_(model.parameters(), clip); optimizer.step()          # OAG/train_paper_field.py:251-252

`np_adamw_step` is the definition (float64 numpy); `AdamW` is the torch.optim.Optimizer that runs it on a ROCm GPU.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

__all__ = ["AdamW", "np_adamw_step", "chunk_table"]

_ROW = 8                      # uint64 words of a table row: hgt_optim_tensor and hgt_optim_group are 64 bytes each
_RING = 4                     # pinned staging slots


def np_adamw_step(params, grads, exp_avg, exp_avg_sq, steps, groups, max_norm=None):
    """The rule of AdamW.step in float64.

    params, exp_avg, exp_avg_sq: lists of arrays; grads: a list of arrays or None (no gradient this step: the tensor is skipped entirely
    -- no decay, no state change, no step count); steps: the tensors' step counts BEFORE this step; groups: dicts with "params" (indices
    into the lists), lr, betas, eps, weight_decay and optionally maximize (False) and clip (True).  With max_norm, the gradients of the
    groups with clip are scaled by min(1, max_norm / (total_norm + 1e-6)), total_norm the 2-norm of all of them together, as
    torch.nn.utils.clip_grad_norm_ does; a NaN or infinite norm gives what that expression gives.  Nothing is modified in place.
    -> (params, exp_avg, exp_avg_sq, steps, total_norm or None)"""
    f64 = lambda a: np.array(a, dtype=np.float64)
    p_out, m_out, v_out, s_out = [f64(a) for a in params], [f64(a) for a in exp_avg], [f64(a) for a in exp_avg_sq], list(steps)
    total_norm, coef = None, 1.0
    with np.errstate(all="ignore"):
        if max_norm is not None:
            sq = 0.0
            for grp in groups:
                if grp.get("clip", True):
                    for i in grp["params"]:
                        if grads[i] is not None:
                            sq += np.sum(f64(grads[i]) ** 2)
            total_norm = np.sqrt(np.float64(sq))
            coef = np.float64(max_norm) / (total_norm + 1e-6)
            coef = np.float64(1.0) if coef > 1.0 else coef                        # a NaN stays a NaN
        for grp in groups:
            lr, (b1, b2), eps, wd = grp["lr"], grp["betas"], grp["eps"], grp["weight_decay"]
            for i in grp["params"]:
                if grads[i] is None:
                    continue
                g = f64(grads[i])
                if max_norm is not None and grp.get("clip", True):
                    g = g * coef
                if grp.get("maximize", False):
                    g = -g
                s_out[i] = step = steps[i] + 1
                p = p_out[i] * (1.0 - lr * wd)
                m = b1 * m_out[i] + (1.0 - b1) * g
                v = b2 * v_out[i] + (1.0 - b2) * g * g
                bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
                p_out[i] = p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
                m_out[i], v_out[i] = m, v
    return p_out, m_out, v_out, s_out, total_norm


def chunk_table(numels):
    """The chunk table of hgt_optim_chunk_table for tensors of these sizes -> (row [n_chunks] int32, first [n_chunks] int64).  Host only."""
    lib = _lib.load()
    numel = np.ascontiguousarray(numels, dtype=np.int64)
    n = C.c_int64()
    _lib.check(lib.hgt_optim_chunk_table(numel.ctypes.data, numel.size, None, 0, C.byref(n)), "hgt_optim_chunk_table")
    table = np.zeros((n.value, 2), dtype=np.int64)
    _lib.check(lib.hgt_optim_chunk_table(numel.ctypes.data, numel.size, table.ctypes.data, n.value, C.byref(n)), "hgt_optim_chunk_table")
    return (table[:, 1] & 0xFFFFFFFF).astype(np.int32), table[:, 0].copy()


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (amsgrad off) with torch.nn.utils.clip_grad_norm_ in front of it, on this library's kernels.

        opt = pyhgt_amd.AdamW(model.parameters(), lr=1e-3, max_norm=0.5)      # or param groups; a group key clip=False keeps a group's
        loss.backward(); opt.step(); opt.zero_grad()                         # tensors out of the norm and away from the coefficient

    Differences from the torch pair, all deliberate:
      * p.grad is NOT modified: the clipped gradient is formed in registers and never stored.
      * opt.total_norm is the norm of the last step as a device scalar (None without max_norm); reading it is the caller's synchronisation.
      * the bits of the result depend on the gradients alone: fixed summation order, no atomics.
    A parameter whose .grad is None is skipped entirely, as in torch.  State dicts are torch.optim.AdamW's: a checkpoint of either class
    resumes in the other.  Parameters are float32, dense, contiguous and on one device."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False, max_norm=None):
        if amsgrad:
            raise NotImplementedError("pyhgt_amd.AdamW: amsgrad=True is not implemented")
        if isinstance(lr, torch.Tensor):
            raise ValueError("pyhgt_amd.AdamW: lr is a Python number (it rides in the host table)")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("pyhgt_amd.AdamW: invalid hyper-parameter")
        if max_norm is not None and not float(max_norm) >= 0.0:
            raise ValueError("pyhgt_amd.AdamW: max_norm must be a non-negative number or None")
        # torch.optim.AdamW's group keys (so that a state dict of this class loads there and keeps its meaning) plus `clip`
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=maximize, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True, clip=True)
        self.max_norm = None if max_norm is None else float(max_norm)
        self.total_norm = None
        self._plan = None
        self._keep = []
        super().__init__(params, defaults)

    # ------------------------------------------------------------------------------------------------------------ construction checks
    @staticmethod
    def _name(group, gi, pi, p):
        names = group.get("param_names")
        return "parameter '%s'" % names[pi] if names else "parameter %d of group %d (shape %s)" % (pi, gi, tuple(p.shape))

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        gi = len(self.param_groups) - 1
        group = self.param_groups[gi]
        if group.get("amsgrad"):
            raise NotImplementedError("pyhgt_amd.AdamW: amsgrad=True is not implemented")
        for pi, p in enumerate(group["params"]):
            what = self._name(group, gi, pi, p)
            if p.dtype != torch.float32:
                raise TypeError("pyhgt_amd.AdamW: %s is %s; only float32 parameters are supported" % (what, p.dtype))
            if p.layout != torch.strided or not p.is_contiguous():
                raise ValueError("pyhgt_amd.AdamW: %s is not a dense contiguous tensor" % what)
            first = self.param_groups[0]["params"][0]
            if p.device != first.device:
                raise ValueError("pyhgt_amd.AdamW: %s is on %s, the first parameter on %s; one optimizer serves one device"
                                 % (what, p.device, first.device))
        self._plan = None

    # ------------------------------------------------------------------------------------------------------------ state dicts
    def state_dict(self):
        """torch.optim.AdamW's format: state[i] = {"step": CPU float tensor, "exp_avg", "exp_avg_sq"}; the step counts are Python integers
        everywhere else and become tensors only here."""
        sd = super().state_dict()
        # (a parameter that never had a gradient has no state, as in torch; an empty entry is left out of the checkpoint)
        sd["state"] = {k: dict(v, step=torch.tensor(float(v["step"]), dtype=torch.float32)) for k, v in sd["state"].items() if v}
        return sd

    def load_state_dict(self, state_dict):
        clip = [group.get("clip", True) for group in self.param_groups]
        super().load_state_dict(state_dict)
        for group, saved, mine in zip(self.param_groups, state_dict["param_groups"], clip):
            if "clip" not in saved:                     # a checkpoint of torch.optim.AdamW: the groups keep what they were built with
                group["clip"] = mine
        self._after_load()

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("max_norm", None)
        self.__dict__.setdefault("total_norm", None)
        self._plan, self._keep = None, []
        self._after_load()

    def _after_load(self):
        for gi, group in enumerate(self.param_groups):
            group.setdefault("clip", True)
            group.setdefault("maximize", False)
            if group.get("amsgrad"):
                raise NotImplementedError("pyhgt_amd.AdamW: amsgrad=True is not implemented")
            for p in group["params"]:
                st = self.state.get(p)
                if st:
                    st["step"] = int(st["step"].item() if torch.is_tensor(st["step"]) else st["step"])
                    st.pop("max_exp_avg_sq", None)
        self._plan = None

    def invalidate(self):
        """Rebuild the device tables at the next step.  Needed only after replacing a state tensor by hand: a moved or re-allocated
        parameter, load_state_dict and add_param_group are noticed without it."""
        self._plan = None

    # ------------------------------------------------------------------------------------------------------------ the tables
    def _build_plan(self, dev):
        """everything that does not change from step to step: rows, state tensors, the chunk table on the device, the staging ring"""
        lib = _lib.load()
        # [parameter, its state dict or None before its first gradient, group index]; (group index, index in the group).  The state
        # is read without inserting: Optimizer.state is a defaultdict, and a parameter without a gradient has no entry, as in torch
        rows, where = [], []
        for gi, group in enumerate(self.param_groups):
            for pi, p in enumerate(group["params"]):
                rows.append([p, self.state.get(p) or None, gi])
                where.append((gi, pi))
        n, n_groups = len(rows), len(self.param_groups)
        numel = np.array([p.numel() for p, _, _ in rows], dtype=np.int64)
        cnt = C.c_int64()
        _lib.check(lib.hgt_optim_chunk_table(numel.ctypes.data, n, None, 0, C.byref(cnt)), "hgt_optim_chunk_table")
        n_chunks = cnt.value
        sizes = [C.c_uint64() for _ in range(4)]
        _lib.check(lib.hgt_optim_tables_bytes(n, n_groups, n_chunks, *[C.byref(s) for s in sizes]), "hgt_optim_tables_bytes")
        step_bytes, groups_off, chunk_bytes, partials_bytes = [s.value for s in sizes]
        chunks_host = torch.zeros(max(chunk_bytes, 16), dtype=torch.uint8).pin_memory()
        _lib.check(lib.hgt_optim_chunk_table(numel.ctypes.data, n, chunks_host.data_ptr(), n_chunks, C.byref(cnt)), "hgt_optim_chunk_table")
        plan = dict(rows=rows, n=n, n_groups=n_groups, n_chunks=n_chunks, dev=dev, groups_off=groups_off,
                    chunks=chunks_host.to(dev, non_blocking=True), chunks_host=chunks_host,      # (pinned, kept: the copy is asynchronous)
                    partials=torch.zeros(max(partials_bytes // 8, 1), dtype=torch.float64, device=dev),
                    norm=torch.zeros((), dtype=torch.float32, device=dev), slot=0,
                    pinned=[torch.zeros(max(step_bytes, 64), dtype=torch.uint8).pin_memory() for _ in range(_RING)],
                    table=[torch.zeros(max(step_bytes, 64), dtype=torch.uint8, device=dev) for _ in range(_RING)],
                    event=[None] * _RING, numel=numel, pptr=[0] * n, where=where,
                    grp=np.array([gi for gi, _ in where], dtype=np.uint64))
        plan["host"] = [t.numpy().view(np.uint64) for t in plan["pinned"]]
        plan["static"] = np.zeros((n, _ROW), dtype=np.uint64)                     # p, -, m, v, numel, group | step << 32, aligned, 0
        plan["static"][:, 4] = numel.astype(np.uint64)
        for r in range(n):
            self._bind_row(plan, r)
        return plan

    def _bind_row(self, plan, r):
        """the pointers of row r that outlive a step: the parameter and, once it has state, its moments"""
        p, st, _ = plan["rows"][r]
        plan["pptr"][r] = p.data_ptr()
        plan["static"][r, 0] = p.data_ptr()
        if st:
            for col, key in ((2, "exp_avg"), (3, "exp_avg_sq")):
                t = st[key]
                if t.device != p.device or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
                    t = st[key] = t.to(device=p.device, dtype=torch.float32).contiguous().reshape(p.shape)
                plan["static"][r, col] = t.data_ptr()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        first = next((p for g in self.param_groups for p in g["params"]), None)
        if first is None:
            return loss
        if not first.is_cuda:
            for gi, group in enumerate(self.param_groups):
                for pi, p in enumerate(group["params"]):
                    if p.grad is not None and p.grad.layout is not torch.strided:
                        raise RuntimeError("pyhgt_amd.AdamW: %s has a sparse gradient; sparse gradients are not supported"
                                           % self._name(group, gi, pi, p))
            raise RuntimeError("pyhgt_amd: AdamW.step runs only on a ROCm GPU tensor; np_adamw_step is the definition on the host")
        dev = first.device
        plan = self._plan
        if plan is None or plan["dev"] != dev:
            plan = self._plan = self._build_plan(dev)
        lib, n = _lib.load(), plan["n"]
        self._keep = keep = []                          # contiguous copies of strided gradients, alive until the next step
        gptr, steps, updated, todo = [0] * n, [0] * n, [], []
        pptr = plan["pptr"]
        for r, (p, st, gi) in enumerate(plan["rows"]):  # every gradient is checked before any state or step count changes
            g = p.grad
            if g is None:
                continue
            if g.layout is not torch.strided:
                raise RuntimeError("pyhgt_amd.AdamW: %s has a sparse gradient; sparse gradients are not supported"
                                   % self._name(self.param_groups[gi], gi, plan["where"][r][1], p))
            if g.dtype is not torch.float32 or g.device != dev:
                raise RuntimeError("pyhgt_amd.AdamW: the gradient of %s is %s on %s; float32 on %s is expected"
                                   % (self._name(self.param_groups[gi], gi, plan["where"][r][1], p), g.dtype, g.device, dev))
            if p.data_ptr() != pptr[r] and (p.device != dev or not p.is_contiguous() or p.dtype != torch.float32):
                self._plan = None
                raise RuntimeError("pyhgt_amd.AdamW: a parameter changed device, dtype or layout under the optimizer; call step() again "
                                   "once all parameters are float32, contiguous and on one device")
            if not g.is_contiguous():
                g = g.contiguous()
                keep.append(g)
            todo.append((r, g))
        if not todo:                                    # no gradient anywhere: nothing moves, and the norm of this step is 0
            if self.max_norm is not None:
                with torch.cuda.device(dev):
                    _lib.check(lib.hgt_grad_norm_join(None, 0, plan["norm"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                               "hgt_grad_norm_join")
                self.total_norm = plan["norm"]
            return loss
        for r, g in todo:
            row = plan["rows"][r]
            p, st = row[0], row[1]
            if st is None:                              # first gradient of this tensor: torch's lazy state
                st = row[1] = self.state[p]
                st["step"] = 0
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                self._bind_row(plan, r)
            elif p.data_ptr() != pptr[r]:               # the parameter moved (model.to(), p.data = ...)
                self._bind_row(plan, r)
            st["step"] = steps[r] = st["step"] + 1
            gptr[r] = g.data_ptr()
            updated.append(p)

        # ---- one pinned slot, reused only after the kernels that read its device copy have finished
        k = plan["slot"]
        plan["slot"] = (k + 1) % _RING
        ev = plan["event"][k]
        if ev is not None and not ev.query():
            ev.synchronize()
        host = plan["host"][k]
        tab = host[:n * _ROW].reshape(n, _ROW)
        tab[:] = plan["static"]
        tab[:, 1] = gptr
        tab[:, 5] = plan["grp"] | (np.array(steps, dtype=np.uint64) << np.uint64(32))
        tab[:, 6] = ((tab[:, 0] | tab[:, 1] | tab[:, 2] | tab[:, 3]) & np.uint64(15)) == 0
        goff = plan["groups_off"] // 8
        gtab = host[goff:goff + plan["n_groups"] * _ROW].reshape(plan["n_groups"], _ROW)
        gf = gtab.view(np.float64)
        for gi, group in enumerate(self.param_groups):
            gf[gi, 0], gf[gi, 1], gf[gi, 2], gf[gi, 3], gf[gi, 4] = group["lr"], group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"]
            gtab[gi, 5] = (1 if group["maximize"] else 0) | ((1 if group["clip"] else 0) << 32)
            gtab[gi, 6] = gtab[gi, 7] = 0
        table = plan["table"][k]
        stream = torch.cuda.current_stream(dev)
        with torch.cuda.device(dev):
            table.copy_(plan["pinned"][k], non_blocking=True)                    # the step's one host-to-device copy
            T, G, Ch, st_ = table.data_ptr(), table.data_ptr() + plan["groups_off"], plan["chunks"].data_ptr(), stream.cuda_stream
            head = (T, n, G, plan["n_groups"], Ch, plan["n_chunks"])
            norm = None
            if self.max_norm is not None:
                _lib.check(lib.hgt_grad_sqnorm(*head, plan["partials"].data_ptr(), st_), "hgt_grad_sqnorm")
                _lib.check(lib.hgt_grad_norm_join(plan["partials"].data_ptr(), plan["n_chunks"], plan["norm"].data_ptr(), st_), "hgt_grad_norm_join")
                norm = plan["norm"].data_ptr()
                self.total_norm = plan["norm"]
            _lib.check(lib.hgt_adamw_step(*head, norm, self.max_norm or 0.0, st_), "hgt_adamw_step")
            if ev is None:
                ev = plan["event"][k] = torch.cuda.Event()
            ev.record(stream)
        # the kernels wrote through raw pointers: bump the version counters the packed-weight caches of HGTConv / GNN are keyed on
        torch.autograd.graph.increment_version(updated)
        return loss
