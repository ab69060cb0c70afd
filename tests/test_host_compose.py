"""The shared pieces of the Python host: the per-kind op table of _lib (make, op_pointers), engine.Program's composition and
graph replay, engine.PinnedRing, and WeightStore.pack_tables.  CPU tests lower on the emulator; one device test replays."""
import ctypes as C

import pytest
import torch

import emu
import _util

needs_emu = pytest.mark.skipif(not emu.available(), reason="emulator needs x86-64 + ROCm's clang++")

# op kind -> (union member of ssde_op, argument structure), written out from include/ssde.h: a derivation that pairs a kind
# with another member or structure must fail here
MEMBERS = {1: ("conv", "ConvArgs"), 2: ("gn", "GnStatsArgs"), 3: ("fir", "UpfirdnArgs"), 4: ("attn", "AttnArgs"),
           5: ("embed", "EmbedArgs"), 6: ("to_nhwc", "ToNhwcArgs"), 7: ("to_nchw", "ToNchwArgs"), 8: ("bias_act", "BiasActArgs"),
           9: ("sumsq", "SumsqArgs"), 10: ("randn", "RandnArgs"), 11: ("langevin", "LangevinArgs"),
           12: ("predictor", "PredictorArgs"), 13: ("fill", "FillArgs"), 14: ("step_inc", "StepIncArgs"),
           15: ("wgrad", "WgradArgs"), 16: ("colsum", "ColsumArgs"), 17: ("gn_bwd", "GnBwdReduceArgs"),
           18: ("pro_bwd", "PrologueBwdArgs"), 19: ("attn_bwd", "AttnBwdArgs"), 20: ("perturb", "PerturbArgs"),
           21: ("dsm_loss", "DsmLossArgs"), 22: ("sumsq_flat", "SumsqFlatArgs"), 23: ("adam", "AdamArgs"),
           24: ("memset", "MemsetArgs"), 25: ("axpy", "AxpyArgs"), 26: ("pack", "PackArgs"), 27: ("project", "ProjectArgs"),
           28: ("gn_fin", "GnFinalizeArgs"), 29: ("pf_drift", "PfDriftArgs"), 30: ("hutch_div", "HutchDivArgs"),
           31: ("colsum_fin", "ColsumFinishArgs"), 32: ("gn_bwd_fin", "GnBwdFinishArgs"), 33: ("gn_apply", "GnApplyArgs"),
           34: ("gn_apply_bwd", "GnApplyBwdArgs")}


def _small_engine():
    from score_sde_pytorch_amd import engine as E
    from score_sde_pytorch_amd.models import utils as mutils
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(_util.small_config("ncsnpp"))
    _util.load_seeded(model, seed=1)
    return model, E.UNetEngine(model, 2, 16, 16, torch.device("cpu"))


def test_op_table_pairs_every_kind_with_its_member_and_structure():
    from score_sde_pytorch_amd import _lib as L
    assert L._UNION_FIELD == {kind: member for kind, (member, _) in MEMBERS.items()}
    assert [name for name, _ in L._OpUnion._fields_] == [member for member, _ in MEMBERS.values()]
    for kind, (member, args) in MEMBERS.items():
        op = L.make(kind)
        assert op.kind == kind and op.flops_class == 0
        assert type(getattr(op.u, member)) is getattr(L, args) is L.ARGS[kind]
        assert bytes(op)[L.Op.u.offset:] == bytes(C.sizeof(L._OpUnion))          # no field given: all zero
    assert C.sizeof(L.Op) == L.Op.u.offset + max(C.sizeof(getattr(L, a)) for _, a in MEMBERS.values())


def test_make_converts_fields_and_op_pointers_finds_them():
    from score_sde_pytorch_amd import _lib as L
    x, data = torch.zeros(4), torch.zeros(4)
    M = [float(i) for i in range(9)]
    op = L.make(L.OP_PROJECT, x=x, x_mean=None, data=data, n=2, c=3, hw=5, use_matrix=1, M=M, invM=tuple(M))
    a = op.u.project
    assert a.x == x.data_ptr() and a.data == data.data_ptr() and a.x_mean is None and a.mask is None
    assert (a.n, a.c, a.hw, a.use_matrix) == (2, 3, 5, 1) and list(a.M) == M and list(a.invM) == M
    base = L.Op.u.offset
    assert list(L.op_pointers(op)) == [(base + L.ProjectArgs.x.offset, x.data_ptr()), (base + L.ProjectArgs.data.offset, data.data_ptr())]
    assert list(L.op_pointers(L.make(L.OP_PROJECT))) == []
    assert L._op_pointer_offsets(L.OP_STEP_INC) == [base]
    from score_sde_pytorch_amd import plan_export
    assert plan_export._op_pointer_offsets(L.OP_CONV) == L.pointer_offsets(L.ConvArgs, base)


@needs_emu
def test_program_of_and_slicing_reproduce_the_program():
    from score_sde_pytorch_amd import engine as E, _lib as L
    with emu.emulated():
        _, eng = _small_engine()
    p, k = eng.program, eng.program.n // 3
    assert len(p[:k]) == k and all(isinstance(op, L.Op) for op in p[:k]) and isinstance(p[:k], list)
    for parts in ([p[:k], p[k:]], [p], [p[:1], p[1:k], p[k:k], p[k:]]):
        q = E.Program.of(parts, eng)
        assert q.n == p.n and bytes(q.ops) == bytes(p.ops)
        assert q.classes == list(p.classes) and q.flops == list(p.flops)
    assert any(c != E.FC_OTHER for c in p.classes) and sum(p.flops) > 0
    # parts that carry neither: a single op, a plain list of ops
    tail = L.make(L.OP_STEP_INC, step_ptr=torch.zeros(1, dtype=torch.int32), delta=1)
    q = E.Program.of([tail, p[:k], list(p[k:k + 2]), [tail]], eng)
    assert bytes(q.ops) == bytes(tail) + bytes(p.ops)[:(k + 2) * C.sizeof(L.Op)] + bytes(tail)
    assert q.classes == [E.FC_OTHER] + list(p.classes[:k]) + [E.FC_OTHER] * 3
    assert q.flops == [0.0] + list(p.flops[:k]) + [0.0] * 3


def test_pinned_ring_delivers_uploads_in_order():
    from score_sde_pytorch_amd import engine as E
    ring = E.PinnedRing(2, 3, torch.float32)
    dst, seen = torch.zeros(3), []
    for v in (1.0, 2.0, 3.0, 4.0, 5.0):
        ring.upload(dst, lambda h, v=v: h.fill_(v))
        seen.append(dst.clone())
    assert [s.tolist() for s in seen] == [[v] * 3 for v in (1.0, 2.0, 3.0, 4.0, 5.0)]
    assert len(ring.bufs) == 2 and ring.bufs[0].tolist() == [5.0] * 3 and ring.bufs[1].tolist() == [4.0] * 3
    assert not E.PinnedRing(1, 24, torch.uint8, pinned=False).bufs[0].is_pinned()


@needs_emu
def test_pack_tables_are_rebuilt_only_when_a_source_moves():
    from score_sde_pytorch_amd import _lib as L
    with emu.emulated():
        model, eng = _small_engine()
    ws = eng.weights
    tables = ws.pack_tables()
    assert tables and ws.pack_tables() is tables
    assert [int(op.kind) for op in ws.pack_ops()] == [L.OP_PACK] * len(tables)
    assert [op.u.pack.table for op in ws.pack_ops()] == [raw.data_ptr() for _, raw in tables]
    w = model.all_modules[3].weight                                    # first conv: a source of an entry with a recipe
    assert any(src is w for e in ws.entries if e.recipe is not None for src in e.sources)
    with torch.no_grad():
        w.add_(1.0)                                                    # new values at the same address: same tables
    assert ws.pack_tables() is tables
    old = w.data
    w.data = old.clone()                                               # the parameter now lives at another address
    assert w.data_ptr() != old.data_ptr()
    moved = ws.pack_tables()
    assert moved is not tables and ws.pack_tables() is moved and len(moved) == len(tables)


@pytest.mark.gpu
def test_replay_from_current_equals_eager_runs():
    """FILL from a 4-entry table + STEP_INC, n = 8, three replays on a side stream issued from the default stream: the smallest
    program whose result depends on the capture having happened and on the side stream being ordered behind the default
    stream's writes (the reset of dst and of the counter) and in front of its reads"""
    from score_sde_pytorch_amd import engine as E, _lib as L
    dev = torch.device("cuda")
    tab = torch.tensor([3.0, 5.0, 7.0, 11.0], device=dev)
    dst = torch.empty(8, device=dev)
    step = torch.empty(1, dtype=torch.int32, device=dev)
    prog = E.Program.of([L.make(L.OP_FILL, dst=dst, tab=tab, step_ptr=step, n=8), L.make(L.OP_STEP_INC, step_ptr=step, delta=1)],
                        (tab, dst, step))
    side = torch.cuda.Stream(device=dev)
    assert torch.cuda.current_stream().cuda_stream != side.cuda_stream

    def reset():
        dst.fill_(-1.0)
        step.zero_()
    reset()
    assert prog._graph is None
    prog.replay_from_current(side, times=3)
    got = (dst.clone(), step.clone())                                  # default stream: must come after the replays
    assert prog._graph is not None
    reset()
    for _ in range(3):
        prog.run()
    want = (dst.clone(), step.clone())
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert want[0].tolist() == [7.0] * 8 and int(want[1]) == 3
    graph = prog._graph
    reset()
    prog.replay_from_current(side)                                     # a second call replays the same graph
    assert prog._graph is graph and dst.tolist() == [3.0] * 8 and int(step) == 1
