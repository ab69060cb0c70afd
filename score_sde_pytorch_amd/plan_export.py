"""Serialise a lowered program as a position-independent PLAN BLOB for hosts without Python (include/ssde.h, "plans";
loader and runner: csrc/plan.hip -> ssde_plan_load, ssde_unet_forward, ssde_pc_reset / ssde_pc_run / ssde_pc_state,
ssde_pc_set_known / ssde_pc_reset_known / ssde_pc_set_noise (inpainting, colorization), ssde_ode_reset / ssde_ode_eval / ssde_ode_solve / ssde_ode_state).

The lowering of NCSNpp.forward (reference models/ncsnpp.py:232-381) and of the predictor-corrector loop body
(sampling.py:403-407) exists once, in engine.py / pc_engine.py.  This module walks what that lowering produced:

  * every tensor the program can point into (activation arena, static I/O, packed kernel-layout weights, the
    reference-layout parameters, embedding / step tables, sampler state, the device-side re-pack descriptor tables)
    becomes a REGION (one per torch storage; constant regions carry their bytes);
  * every pointer field of every `ssde_op` -- found through the ctypes mirror of include/ssde.h -- is zeroed and
    recorded as a relocation (region, byte offset); the same for the src / src2 / dst pointers inside the re-pack tables;
  * parameters are listed with their state_dict names so that a host can overwrite them from a checkpoint and call
    ssde_plan_refresh_weights (four device launches re-pack every kernel-layout copy).

Export needs no GPU: a program lowered on 'cpu' (dry lowering) serialises the same way.
"""
import bisect
import ctypes as C
import struct

import torch

from . import _lib as L
from . import engine as E

MAGIC = b"SSDEPLN1"
REGION_ZERO, REGION_CONST = 0, 1
RELOC_OP, RELOC_REFRESH_OP, RELOC_REGION = 0, 1, 2
PLAN_UNET, PLAN_PC, PLAN_TRAIN, PLAN_ODE, PLAN_LIKELIHOOD = 0, 1, 2, 3, 4
IO_X, IO_COND, IO_SIGMA, IO_STD, IO_OUT, IO_XMEAN, IO_STEP, IO_SEED = range(8)
(IO_BATCH, IO_Z, IO_A, IO_S, IO_G2, IO_LOSS, IO_HYPER, IO_DROP_SEED, IO_GOUT, IO_GX, IO_GRAD, IO_PARAMS) = range(8, 20)
IO_ODE_DYN, IO_ODE_K, IO_ODE_STATE, IO_ODE_PROBE = range(20, 24)
IO_SLOTS = 24
ODE_PARTIALS = 1024                      # include/ssde.h: SSDE_ODE_PARTIALS
ODE_METHODS = {"RK45": 0, "RK23": 1, "DOP853": 2}   # include/ssde.h: SSDE_ODE_*
PC_PROJ_NONE, PC_PROJ_MASK, PC_PROJ_COLOR = 0, 1, 2  # include/ssde.h: SSDE_PC_PROJ_*


class PlanHeader(C.Structure):
    _fields_ = [("magic", C.c_char * 8), ("abi_version", C.c_int32), ("sizeof_op", C.c_int32),
                ("n_regions", C.c_int32), ("n_ops", C.c_int32), ("n_refresh_ops", C.c_int32), ("n_relocs", C.c_int32),
                ("n_params", C.c_int32), ("kind", C.c_int32),
                ("batch", C.c_int32), ("channels", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("nfe_per_iteration", C.c_int32), ("sde_steps", C.c_int32), ("io", C.c_int32 * IO_SLOTS), ("seg", C.c_int32 * 4),
                ("n_flat", C.c_int64), ("data_bytes", C.c_int64)]


class PlanRegion(C.Structure):
    _fields_ = [("bytes", C.c_int64), ("data_offset", C.c_int64), ("kind", C.c_int32), ("_pad0", C.c_int32), ("name", C.c_char * 32)]


class PlanReloc(C.Structure):
    _fields_ = [("target_kind", C.c_int32), ("target", C.c_int32), ("byte_offset", C.c_int64), ("region", C.c_int32),
                ("_pad0", C.c_int32), ("offset", C.c_int64)]


class PlanParam(C.Structure):
    _fields_ = [("name", C.c_char * 96), ("region", C.c_int32), ("_pad0", C.c_int32), ("offset", C.c_int64), ("numel", C.c_int64)]


_op_pointer_offsets = L._op_pointer_offsets      # byte offset of every pointer field of an op of a kind


class _Regions:
    """Torch storages the program points into; lookup of an address -> (region id, byte offset)."""

    def __init__(self):
        self.by_ptr, self.list = {}, []      # storage data_ptr -> id ; [dict(ptr, bytes, kind, name, storage_tensor)]

    def add(self, t, kind, name, own=False):
        """own=True: a tensor that is a piece of a larger storage becomes a region of its own extent (a parameter that a
        training engine has since moved into its flat buffer exports as it did before the move)"""
        if t is None:
            return None
        st = t.untyped_storage()
        key, nbytes, piece = st.data_ptr(), st.nbytes(), False
        if own and t.is_contiguous() and (t.data_ptr() != key or t.numel() * t.element_size() != nbytes):
            key, nbytes, piece = t.data_ptr(), t.numel() * t.element_size(), True
        if key in self.by_ptr:
            r = self.list[self.by_ptr[key]]
            r["kind"] = max(r["kind"], kind)
            return self.by_ptr[key]
        self.by_ptr[key] = len(self.list)
        self.list.append(dict(ptr=key, bytes=nbytes, kind=kind, name=name, keep=t, piece=piece))
        return len(self.list) - 1

    def freeze(self):
        self._starts = sorted((r["ptr"], i) for i, r in enumerate(self.list))
        self._keys = [s for s, _ in self._starts]

    def find(self, addr):
        i = bisect.bisect_right(self._keys, addr) - 1
        if i >= 0:
            rid = self._starts[i][1]
            r = self.list[rid]
            if r["ptr"] <= addr <= r["ptr"] + r["bytes"]:
                return rid, addr - r["ptr"]
        raise ValueError("plan export: pointer 0x%x lies in no known tensor" % addr)

    def data(self, rid):
        r = self.list[rid]
        t = r["keep"]
        if r["piece"]:
            return t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy().tobytes()
        flat = torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage().cpu() if t.is_cuda else t.untyped_storage())
        return bytes(flat.numpy().tobytes())


def _collect_unet(regions, eng):
    for i, blk in enumerate(eng.b.blocks):
        regions.add(blk, REGION_ZERO, "arena%d" % i)
    for i, t in enumerate(eng.b.keep):
        regions.add(t, REGION_CONST, "table%d" % i)
    # An inference engine on a model whose parameters a training engine has flattened since (backward.FlatParams: views into
    # one buffer) exports one region per parameter, as before the move: the blob of an engine does not depend on what was
    # built on its model afterwards.  A training engine exports its own flat buffer whole.
    own = getattr(eng, "flat", None) is None
    for i, e in enumerate(eng.weights.entries):
        regions.add(e.packed, REGION_CONST, "packed%d" % i)
        for s in e.sources:
            regions.add(s.detach(), REGION_CONST, "param", own=own)
    for i, (_, raw) in enumerate(eng.weights.pack_tables()):
        regions.add(raw, REGION_CONST, "packtab%d" % i)


def _emit(kind, regions, ops, n_ops, eng_unet, model, io_tensors, batch, shape, nfe, sde_steps, seg=(0, 0, 0, 0), n_flat=0):
    regions.freeze()
    relocs = []

    def relocate(raw, offsets, target_kind, index, base=0):
        """zero every pointer of `raw` at base + offsets and record it as a relocation of target (target_kind, index)"""
        for off, addr in L.pointers_at(raw, offsets, base):
            relocs.append((target_kind, index, off) + regions.find(addr))
            struct.pack_into("<Q", raw, off, 0)
        return raw

    op_bytes = bytearray()
    for i in range(n_ops):
        op_bytes += relocate(bytearray(bytes(ops[i])), _op_pointer_offsets(int(ops[i].kind)), RELOC_OP, i)
    # ---- weight refresh program: one ssde_pack_weights launch per descriptor table
    refresh = bytearray()
    tables = eng_unet.weights.pack_tables()
    desc_ptrs = L.pointer_offsets(L.PackDesc)
    table_patches = {}
    for j, ((args, raw_t), op) in enumerate(zip(tables, eng_unet.weights.pack_ops())):
        refresh += relocate(bytearray(bytes(op)), _op_pointer_offsets(L.OP_PACK), RELOC_REFRESH_OP, j)
        # pointers inside the table
        tid, toff0 = regions.find(raw_t.data_ptr())
        tb = bytearray(regions.data(tid))
        for d in range(int(args.count)):
            relocate(tb, desc_ptrs, RELOC_REGION, tid, toff0 + d * C.sizeof(L.PackDesc))
        table_patches[tid] = bytes(tb)
    # ---- parameters by state_dict name
    params = []
    for name, p in model.named_parameters():
        try:
            rid, roff = regions.find(p.data_ptr())
        except ValueError:
            continue                                    # a parameter no kernel reads (none today)
        params.append((name, rid, roff, p.numel()))
    # ---- data section
    data = bytearray()
    reg_structs = []
    for rid, r in enumerate(regions.list):
        rs = PlanRegion()
        rs.bytes, rs.kind, rs.name = r["bytes"], r["kind"], r["name"].encode()[:31]
        rs.data_offset = -1
        if r["kind"] == REGION_CONST:
            while len(data) % 16:
                data.append(0)
            rs.data_offset = len(data)
            data += table_patches.get(rid) or regions.data(rid)
        reg_structs.append(rs)
    hdr = PlanHeader()
    hdr.magic, hdr.abi_version, hdr.sizeof_op = MAGIC, L.ABI_VERSION, C.sizeof(L.Op)
    hdr.n_regions, hdr.n_ops, hdr.n_refresh_ops, hdr.n_relocs, hdr.n_params = len(reg_structs), n_ops, len(tables), len(relocs), len(params)
    hdr.kind, hdr.batch = kind, batch
    hdr.channels, hdr.height, hdr.width = shape
    hdr.nfe_per_iteration, hdr.sde_steps = nfe, sde_steps
    for k in range(4):
        hdr.seg[k] = int(seg[k])
    hdr.n_flat = int(n_flat)
    for slot in range(IO_SLOTS):
        t = io_tensors.get(slot)
        hdr.io[slot] = -1
        if t is not None:
            rid, roff = regions.find(t.data_ptr())
            assert roff == 0, "plan I/O tensors must start their storage"
            hdr.io[slot] = rid
    hdr.data_bytes = len(data)
    out = bytearray(bytes(hdr))
    for rs in reg_structs:
        out += bytes(rs)
    out += op_bytes + refresh
    for tk, tgt, boff, rid, roff in relocs:
        q = PlanReloc()
        q.target_kind, q.target, q.byte_offset, q.region, q.offset = tk, tgt, boff, rid, roff
        out += bytes(q)
    for name, rid, roff, numel in params:
        q = PlanParam()
        q.name, q.region, q.offset, q.numel = name.encode()[:95], rid, roff, numel
        out += bytes(q)
    out += data
    return bytes(out)


def export_unet_plan(eng):
    """engine.UNetEngine -> blob for ssde_plan_load / ssde_unet_forward."""
    eng.weights.refresh()
    regions = _Regions()
    _collect_unet(regions, eng)
    io = {IO_X: eng.x_in.tensor, IO_COND: eng.cond.tensor, IO_OUT: eng.out.tensor}
    if eng.sig is not eng.cond:
        io[IO_SIGMA] = eng.sig.tensor
    if eng.std is not None:
        io[IO_STD] = eng.std.tensor
    return _emit(PLAN_UNET, regions, eng.program.ops, eng.program.n, eng, eng.model, io, eng.n, (eng.channels, eng.h, eng.w), 1, 0)


def export_pc_plan(sampler, with_rng=True):
    """pc_engine.FusedPCSampler -> blob for ssde_pc_reset / ssde_pc_run / ssde_pc_state (one program = one PC iteration).

    The engine of an inpainter / colorizer (controllable_generation: fn.engine(model, shape)) exports the same way; its
    iteration holds the SSDE_OP_PROJECT ops through which ssde_pc_set_known / ssde_pc_reset_known find the known-data and mask
    regions.  with_rng=False leaves the noise to the host: ssde_pc_set_noise before every iteration."""
    eng = sampler.unet
    eng.weights.refresh()
    prog = sampler.step_program(with_rng=with_rng)
    regions = _Regions()
    _collect_unet(regions, eng)
    for name in ("x_mean", "z_c", "z_p", "gss", "zss", "step", "seed_word", "proj_data", "proj_mask", "z_pc", "z_pp"):
        t = getattr(sampler, name, None)
        if t is not None:
            regions.add(t, REGION_ZERO, name)
    for k, t in sampler.tabs.items():
        regions.add(t, REGION_CONST, "tab_" + k)
    io = {IO_X: eng.x_in.tensor, IO_COND: eng.cond.tensor, IO_OUT: eng.out.tensor, IO_XMEAN: sampler.x_mean,
          IO_STEP: sampler.step, IO_SEED: sampler.seed_word}
    if eng.std is not None:
        io[IO_STD] = eng.std.tensor
    B, Cc, H, W = sampler.shape
    return _emit(PLAN_PC, regions, prog.ops, prog.n, eng, sampler.model, io, B, (Cc, H, W), sampler.nfe_per_step(), sampler.sde.N)


def export_train_plan(fs, optimizer=None, ema=None):
    """losses.FusedTrainStep -> blob for ssde_train_step / ssde_train_forward / ssde_unet_backward.

    One op array: [perturb | forward | loss head | backward | clip + Adam + EMA]; the segment starts go into the
    header.  The flat parameter buffer (the parameters are views into it), the flat gradient, Adam's moments and the EMA
    shadow are regions of their own; moments and shadow carry their CURRENT contents, so a plan exported mid-run resumes.
    Without `optimizer` the plan stops after the backward segment (hosts that bring their own optimizer read the flat
    gradient through ssde_unet_backward)."""
    eng = fs.eng
    eng.weights.refresh()
    regions = _Regions()
    _collect_unet(regions, eng)
    regions.add(fs.flat.data, REGION_CONST, "flat_params")
    regions.add(fs.flat.grad, REGION_ZERO, "flat_grad")
    for name in ("z", "batch", "a", "s", "g2", "losses", "loss", "hyper", "gnorm", "partial"):
        regions.add(getattr(fs, name), REGION_ZERO, name)
    parts = [fs._head[0], eng.program[:eng.n_fwd], fs._head[1], eng.program[eng.n_fwd:]]
    seg0 = fs._head[0].n
    seg1 = seg0 + eng.n_fwd
    seg2 = seg1 + fs._head[1].n
    seg3 = 0
    if optimizer is not None:
        m, v = optimizer.flatten_like(fs.flat)
        regions.add(m, REGION_CONST, "adam_m")
        regions.add(v, REGION_CONST, "adam_v")
        if ema is not None:
            regions.add(ema.flatten_like(fs.flat), REGION_CONST, "ema")
        seg3 = seg2 + eng.program.n - eng.n_fwd
        parts.append(fs._optimizer_program(optimizer, ema))
    prog = E.Program.of(parts, fs)
    io = {IO_X: eng.x_in.tensor, IO_COND: eng.cond.tensor, IO_OUT: eng.out.tensor, IO_BATCH: fs.batch, IO_Z: fs.z, IO_A: fs.a,
          IO_S: fs.s, IO_LOSS: fs.loss, IO_HYPER: fs.hyper, IO_GOUT: eng.gout.tensor, IO_GRAD: fs.flat.grad, IO_PARAMS: fs.flat.data}
    if fs.spec["likelihood_weighting"]:
        io[IO_G2] = fs.g2
    if eng.sig is not eng.cond:
        io[IO_SIGMA] = eng.sig.tensor
    if eng.std is not None:
        io[IO_STD] = eng.std.tensor
    if eng.drop_seed is not None:
        io[IO_DROP_SEED] = eng.drop_seed
    if eng.gx is not None:
        io[IO_GX] = eng.gx.tensor
    return _emit(PLAN_TRAIN, regions, prog.ops, prog.n, eng, fs.model, io, eng.n, (eng.channels, eng.h, eng.w), 1, 0,
                 seg=(seg0, seg1, seg2, seg3), n_flat=fs.flat.numel)


def export_ode_plan(rhs, method="RK45"):
    """ode.FusedDrift / ode.FusedLikelihoodRhs -> blob for ssde_ode_reset / ssde_ode_eval / ssde_ode_solve[_method] /
    ssde_ode_state (one program = one evaluation of the right-hand side, its scalars read from the `dyn` record).

    Besides the U-Net's regions the blob names the solver state as zero regions: the record, the fp64 slope rows -- the
    n_stages + 1 of `method` (ode.TABLEAUS) and never fewer than the 7 of RK45, so every blob runs RK45 and RK23 and the
    default blob is what it always was --, and one block holding y, y_new, the stage argument and the error-norm partials and result (offsets: include/ssde.h,
    SSDE_IO_ODE_STATE).  State length: B*C*H*W for the sampler, plus B log-density terms for the likelihood, whose plan also
    carries the probe (set per solve by ssde_ode_reset, which copies it into the cotangent buffer too)."""
    from . import ode
    if not isinstance(rhs, (ode.FusedDrift, ode.FusedLikelihoodRhs)):
        raise TypeError("export_ode_plan: expected an ode.FusedDrift or an ode.FusedLikelihoodRhs, got %s" % type(rhs).__name__)
    if method not in ode.TABLEAUS:
        raise ValueError("export_ode_plan: method must be one of %s, got %r" % (sorted(ode.TABLEAUS), method))
    rows = max(7, ode.TABLEAUS[method]["n_stages"] + 1)
    eng = rhs.unet
    eng.weights.refresh()
    lik = isinstance(rhs, ode.FusedLikelihoodRhs)
    B, Cc, H, W = rhs.shape
    n_state = rhs.n + (B if lik else 0)
    regions = _Regions()
    _collect_unet(regions, eng)
    slopes = torch.zeros(rows * n_state, dtype=torch.float64, device=rhs.dyn.device)
    state = torch.zeros(3 * n_state + ODE_PARTIALS + 1, dtype=torch.float64, device=rhs.dyn.device)
    regions.add(rhs.dyn, REGION_ZERO, "ode_dyn")
    regions.add(slopes, REGION_ZERO, "ode_slopes")
    regions.add(state, REGION_ZERO, "ode_state")
    io = {IO_X: eng.x_in.tensor, IO_COND: eng.cond.tensor, IO_OUT: eng.out.tensor, IO_ODE_DYN: rhs.dyn, IO_ODE_K: slopes,
          IO_ODE_STATE: state}
    if eng.sig is not eng.cond:
        io[IO_SIGMA] = eng.sig.tensor
    if eng.std is not None:
        io[IO_STD] = eng.std.tensor
    if lik:
        regions.add(rhs.eps, REGION_ZERO, "ode_probe")
        io.update({IO_ODE_PROBE: rhs.eps, IO_GOUT: eng.gout.tensor, IO_GX: eng.gx.tensor})
    return _emit(PLAN_LIKELIHOOD if lik else PLAN_ODE, regions, rhs.program.ops, rhs.program.n, eng, eng.model, io, B, (Cc, H, W), 1, 0)


# ---------------------------------------------------------------------------------------------------------------------
# ctypes binding of the plan entry points (what a C host calls; used by the tests and by tools)
def bind(lib):
    lib.ssde_plan_load.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
    lib.ssde_plan_load_file.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    lib.ssde_plan_destroy.argtypes = [C.c_void_p]
    lib.ssde_plan_info.argtypes = [C.c_void_p, C.POINTER(PlanHeader)]
    lib.ssde_plan_param.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_char_p)]
    lib.ssde_plan_refresh_weights.argtypes = [C.c_void_p, C.c_void_p]
    lib.ssde_unet_forward.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_void_p]
    lib.ssde_pc_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.ssde_pc_run.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.ssde_pc_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ssde_pc_projection.argtypes = [C.c_void_p]
    lib.ssde_pc_set_known.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ssde_pc_reset_known.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.ssde_pc_set_noise.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.ssde_train_step.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.POINTER(C.c_float), C.c_uint32, C.c_void_p, C.c_void_p]
    lib.ssde_train_forward.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_void_p]
    lib.ssde_unet_backward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ssde_plan_copy_io.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    lib.ssde_ode_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ssde_ode_eval.argtypes = [C.c_void_p, C.c_double, ODE_SCALARS_FN, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ssde_ode_solve.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, ODE_SCALARS_FN, C.c_void_p, C.c_int32,
                                   C.c_int32, C.POINTER(C.c_int32), C.c_void_p]
    lib.ssde_ode_solve_method.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, ODE_SCALARS_FN, C.c_void_p,
                                          C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_void_p]
    lib.ssde_ode_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


# include/ssde.h: ssde_ode_scalars_fn -- (t, user, out[4]) -> 0, or non-zero to abort the solve
ODE_SCALARS_FN = C.CFUNCTYPE(C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_float))


def _ode_callback(scalars):
    """A Python callable t -> (label, second, a, g2) as an ssde_ode_scalars_fn; an exception aborts the solve (return 1)
    and is kept in `.error` of the returned object for the caller to re-raise."""
    def thunk(t, _user, out):
        try:
            v = scalars(t)
            for i in range(4):
                out[i] = v[i]
            return 0
        except Exception as e:      # noqa: BLE001  (must not propagate through the C frames)
            thunk.error = e
            return 1
    thunk.error = None
    fn = ODE_SCALARS_FN(thunk)
    fn.thunk = thunk
    return fn


class LoadedPlan:
    """A plan loaded through the C API (device memory owned by the library)."""

    def __init__(self, blob):
        self.lib = bind(L.load())
        self.handle = C.c_void_p()
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        L.check(self.lib.ssde_plan_load(C.cast(buf, C.c_void_p), len(blob), C.byref(self.handle)), "ssde_plan_load")
        self.header = PlanHeader()
        L.check(self.lib.ssde_plan_info(self.handle, C.byref(self.header)))

    def param(self, name):
        dev, numel = C.c_void_p(), C.c_int64()
        L.check(self.lib.ssde_plan_param(self.handle, name.encode(), -1, C.byref(dev), C.byref(numel), None), "ssde_plan_param")
        return dev.value, numel.value

    def refresh_weights(self, stream=None):
        L.check(self.lib.ssde_plan_refresh_weights(self.handle, C.c_void_p(stream or 0)), "ssde_plan_refresh_weights")

    def unet_forward(self, x, cond, sigma=None, std=None, stream=None):
        out = torch.empty_like(x)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        L.check(self.lib.ssde_unet_forward(self.handle, p(x), p(cond), p(sigma), p(std), p(out), C.c_void_p(stream or 0)), "ssde_unet_forward")
        return out

    # ---- sampler plans (ssde_pc_*): tensors are fp32, contiguous, on the plan's device, and stay alive until `stream` has run
    def pc_reset(self, x_T, seed, stream=None):
        L.check(self.lib.ssde_pc_reset(self.handle, C.c_void_p(x_T.data_ptr()), int(seed), C.c_void_p(stream or 0)), "ssde_pc_reset")

    def pc_run(self, n_iterations, use_graph=False, stream=None):
        L.check(self.lib.ssde_pc_run(self.handle, int(n_iterations), int(bool(use_graph)), C.c_void_p(stream or 0)), "ssde_pc_run")

    def pc_state(self, like, stream=None):
        """(x, x_mean) shaped / placed like `like`"""
        x, x_mean = torch.empty_like(like, dtype=torch.float32), torch.empty_like(like, dtype=torch.float32)
        L.check(self.lib.ssde_pc_state(self.handle, C.c_void_p(x.data_ptr()), C.c_void_p(x_mean.data_ptr()), C.c_void_p(stream or 0)),
                "ssde_pc_state")
        return x, x_mean

    def pc_projection(self):
        """PC_PROJ_NONE, PC_PROJ_MASK (inpainting) or PC_PROJ_COLOR (colorization): what the plan's iteration contains"""
        kind = self.lib.ssde_pc_projection(self.handle)
        if kind < 0:
            L.check(kind, "ssde_pc_projection")
        return kind

    def pc_set_known(self, data, mask=None, stream=None):
        """the known data (model input scaling; colorization: the grey image on all three channels) and the 0 / 1 mask
        (None: the colorizer's own)"""
        L.check(self.lib.ssde_pc_set_known(self.handle, C.c_void_p(data.data_ptr()), C.c_void_p(mask.data_ptr()) if mask is not None else None,
                                           C.c_void_p(stream or 0)), "ssde_pc_set_known")

    def pc_reset_known(self, prior, seed, stream=None):
        """the reference's start state from a prior sample (after pc_set_known); step 0, seed word `seed`"""
        L.check(self.lib.ssde_pc_reset_known(self.handle, C.c_void_p(prior.data_ptr()), int(seed), C.c_void_p(stream or 0)),
                "ssde_pc_reset_known")

    def pc_set_noise(self, which, z, stream=None):
        """plans exported with with_rng=False: which = 0 corrector, 1 predictor, 2 / 3 the projections after them"""
        L.check(self.lib.ssde_pc_set_noise(self.handle, int(which), C.c_void_p(z.data_ptr()), C.c_void_p(stream or 0)), "ssde_pc_set_noise")

    def train_step(self, batch, z, a, s, labels, hyper9, seed, g2=None, stream=None):
        """one optimisation step through the C entry point; returns the loss as a 1-element tensor on the inputs' device"""
        loss = torch.zeros(1, dtype=torch.float32, device=batch.device)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        hy = (C.c_float * 9)(*[float(v) for v in hyper9])
        L.check(self.lib.ssde_train_step(self.handle, p(batch), p(z), p(a), p(s), p(labels), p(g2), hy, int(seed) & 0xFFFFFFFF, p(loss),
                                         C.c_void_p(stream or 0)), "ssde_train_step")
        return loss

    def train_forward(self, x, cond, seed=0, sigma=None, std=None, stream=None):
        out = torch.empty_like(x)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        L.check(self.lib.ssde_train_forward(self.handle, p(x), p(cond), p(sigma), p(std), int(seed) & 0xFFFFFFFF, p(out),
                                            C.c_void_p(stream or 0)), "ssde_train_forward")
        return out

    def unet_backward(self, dout, want_dx=False, stream=None):
        dx = torch.empty_like(dout) if want_dx else None
        dparams = torch.empty(int(self.header.n_flat), dtype=torch.float32, device=dout.device)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        L.check(self.lib.ssde_unet_backward(self.handle, p(dout), p(dx), p(dparams), C.c_void_p(stream or 0)), "ssde_unet_backward")
        return dx, dparams

    def _ode_call(self, what, fn, rc):
        err, fn.thunk.error = fn.thunk.error, None
        if err is not None:
            raise err
        L.check(rc, what)

    def ode_reset(self, x0, probe=None, stream=None):
        """load the initial state (and the probe of a likelihood plan); x0 / probe: fp32 tensors on the plan's device"""
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        x0 = x0.contiguous()
        probe = probe.contiguous() if probe is not None else None
        L.check(self.lib.ssde_ode_reset(self.handle, p(x0), p(probe), C.c_void_p(stream or 0)), "ssde_ode_reset")

    def ode_state_len(self):
        h = self.header
        return h.batch * h.channels * h.height * h.width + (h.batch if h.kind == PLAN_LIKELIHOOD else 0)

    def ode_eval(self, t, scalars, like, stream=None):
        """the right-hand side at the current state and time t: fp64 tensor [n] (sampler) or [n + B] (likelihood) on like's device"""
        out = torch.empty(self.ode_state_len(), dtype=torch.float64, device=like.device)
        fn = _ode_callback(scalars)
        rc = self.lib.ssde_ode_eval(self.handle, float(t), fn, None, C.c_void_p(out.data_ptr()), C.c_void_p(stream or 0))
        self._ode_call("ssde_ode_eval", fn, rc)
        return out

    def ode_solve(self, t0, t1, rtol, atol, scalars, use_graph=False, max_nfev=0, stream=None, method="RK45"):
        """integrate the plan's state from t0 to t1 (the library's adaptive driver; method: a key of ODE_METHODS);
        `scalars`: t -> (label, second, a, g2), e.g. ode.scalars_fn(rhs).  Returns the number of evaluations."""
        if method not in ODE_METHODS:
            raise ValueError("ode_solve: method must be one of %s, got %r" % (sorted(ODE_METHODS), method))
        nfev = C.c_int32(0)
        fn = _ode_callback(scalars)
        rc = self.lib.ssde_ode_solve_method(self.handle, ODE_METHODS[method], float(t0), float(t1), float(rtol), float(atol), fn, None,
                                            int(bool(use_graph)), int(max_nfev), C.byref(nfev), C.c_void_p(stream or 0))
        self._ode_call("ssde_ode_solve_method", fn, rc)
        return int(nfev.value)

    def ode_state(self, like, stream=None):
        """(x shaped / placed like `like` in fp32, delta_logp [B] fp64 or None for a sampler plan)"""
        x = torch.empty_like(like, dtype=torch.float32)
        dl = torch.empty(int(self.header.batch), dtype=torch.float64, device=like.device) if self.header.kind == PLAN_LIKELIHOOD else None
        L.check(self.lib.ssde_ode_state(self.handle, C.c_void_p(x.data_ptr()), C.c_void_p(dl.data_ptr()) if dl is not None else None,
                                        C.c_void_p(stream or 0)), "ssde_ode_state")
        return x, dl

    def read_io(self, slot, like):
        """the first like.numel() elements of an I/O region, as a tensor shaped / typed / placed like `like`"""
        out = torch.empty_like(like)
        L.check(self.lib.ssde_plan_copy_io(self.handle, int(slot), C.c_void_p(out.data_ptr()), out.numel() * out.element_size(), 0,
                                           C.c_void_p(0)), "ssde_plan_copy_io")
        return out

    def close(self):
        if self.handle:
            self.lib.ssde_plan_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
