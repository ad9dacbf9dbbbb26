"""The callback path of ``PTEngine`` lives in ``ptmcmcsampler_amd/callback_path.py`` (the mixin ``CallbackPath``): the
surface it had in engine.py, and the helpers its stages share -- ``_dev_f64`` (a value as a contiguous f64 tensor on the engine's
device), ``_jump_result`` (the return value of a batched jump, custom or auxiliary) -- with the messages to the letter.  Checked without
a GPU and without the library, on engines that never saw their constructor (tests/test_ring_stages.py works the same way); the stages run
against a library that only records its calls.  The runs: tests/test_callback_path_gpu.py."""
import inspect
import re

import numpy as np
import pytest
import torch

from ptmcmcsampler_amd import _lib, callback_path, engine
from ptmcmcsampler_amd.engine import PTEngine

# every method that moved, with the signature it had in engine.py
SIGNATURES = {
    "_cb_values": "(self, v, n=None, what='the callback')",
    "eval_callback": "(self, X, logl, logp)",
    "_logl_in_support": "(self, flat, lp, logl)",
    "init_state_callback": "(self, p0, logl, logp, i0=0)",
    "_cb_grad": "(self, r, n, what)",
    "gradient_stage": "(self, it, logl_grad, logp_grad=None)",
    "jump_stage": "(self, it)",
    "aux_stage": "(self, it)",
    "box_draw_jump": "(self, lo, hi)",
    "split_step": "(self, it, logl, logp, logl_grad=None, logp_grad=None)",
    "builtin_logl": "(self)",
    "builtin_logl_grad": "(self)",
    "builtin_logp": "(self)",
    "builtin_logp_grad": "(self)",
    "dense_logl_callback": "(self, mu, P)",
    "proposals": "(self)",
    "callback_segment": "(self, it, end, logl, logp, logl_grad=None, logp_grad=None)",
    "callback_segment_graph": "(self, it, end, logl, logp)",
    "run_callback": "(self, niter, logl, logp, fused=True, graph=False, logl_grad=None, logp_grad=None)",
    "_rows_callbacks": "(self)",
}
N, D = 3, 2
F64 = torch.float64


# ---------------------------------------------------------------------- surface
@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_every_moved_method_is_the_engine_s_with_its_signature(name):
    assert str(inspect.signature(getattr(PTEngine, name))) == SIGNATURES[name]
    assert getattr(PTEngine, name) is getattr(callback_path.CallbackPath, name)
    assert name not in vars(PTEngine)                                 # one copy: the mixin's


def test_the_engine_module_still_exports_the_box_draw_jump():
    assert engine.box_draw_jump is callback_path.box_draw_jump and engine._BoxDrawJump is callback_path._BoxDrawJump
    assert str(inspect.signature(engine.box_draw_jump)) == "(lo, hi)" and str(inspect.signature(engine._BoxDrawJump)) == "(lo, hi)"
    jump = engine.box_draw_jump(-1.0, [1.0, 2.0])
    assert isinstance(jump, engine._BoxDrawJump) and jump.engine is None and jump.__name__ == "boxDrawJump"
    with pytest.raises(_lib.PtmiError, match="runs inside PTEngine.jump_stage"):
        jump(None, 1, None)                                           # unbound
    e = stub()
    bound = e.box_draw_jump(-1.0, [1.0, 2.0])
    assert bound.engine is e and bound.lo.tolist() == [-1.0, -1.0] and bound.hi.tolist() == [1.0, 2.0]


def test_the_class_defaults_come_through_the_mixin():
    assert PTEngine.logl_in_support is False and PTEngine.jumps_with_grad is False and PTEngine._aux == ()
    assert issubclass(PTEngine, callback_path.CallbackPath)
    for name in ("logl_in_support", "jumps_with_grad", "_aux"):
        assert name in vars(callback_path.CallbackPath) and name not in vars(PTEngine)
    assert "__init__" not in vars(callback_path.CallbackPath) and type(callback_path.CallbackPath) is type


# ---------------------------------------------------------------------- the stub
class FakeLib(object):
    """A library that records ``(name, arguments behind the handle)`` and returns 0; ``ptmi_cj_begin`` lists one function with N rows."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(h, *a):
            self.calls.append((name,) + a)
            if name == "ptmi_cj_begin":
                a[-1][0], a[-1][1] = 0, N
            return 0
        return call

    def names(self):
        return [c[0] for c in self.calls]


def stub(jumps=(), aux=()):
    """A PTEngine that never saw its constructor: N chains of D parameters on the CPU."""
    e = PTEngine.__new__(PTEngine)
    e.device, e.d, e.W, e.nt, e.h, e.lib = torch.device("cpu"), D, N, 1, None, FakeLib()
    e._jumps, e._aux = list(jumps), list(aux)
    e.t = dict(Q=torch.zeros((N, 1, D), dtype=F64), Q2=None, qaux=torch.zeros((N, 1, 4), dtype=F64))
    return e


# ---------------------------------------------------------------------- _dev_f64
def test_dev_f64_hands_back_what_is_ready_and_converts_the_rest():
    e = stub()
    ready = torch.arange(6, dtype=F64).reshape(3, 2)
    assert e._dev_f64(ready) is ready
    row = ready[1]
    assert e._dev_f64(row) is row                                     # a contiguous view is ready too
    base = np.arange(6.0).reshape(3, 2)
    for v in (torch.arange(6, dtype=torch.float32).reshape(3, 2), base, base.tolist(), torch.arange(6, dtype=F64).reshape(2, 3).t()):
        want = np.asarray(v.tolist() if torch.is_tensor(v) else v, dtype=np.float64)
        out = e._dev_f64(v)
        assert torch.is_tensor(out) and out.dtype == F64 and out.device == e.device and out.is_contiguous() and out is not v
        assert out.shape == want.shape and np.array_equal(out.numpy(), want)
    assert not torch.arange(6, dtype=F64).reshape(2, 3).t().is_contiguous()


# ---------------------------------------------------------------------- _jump_result
Q_OK = np.arange(6.0).reshape(N, D)
NOT_A_PAIR = "f must return (Q[n, ndim], qxy[n] or 0 or None)"


@pytest.mark.parametrize("r, msg", [
    (torch.zeros((N, D), dtype=F64), NOT_A_PAIR),
    ((Q_OK, None, None), NOT_A_PAIR),
    ((np.zeros((3, 3)), None), "f returned proposals (3, 3) for 3 rows of 2 parameters"),
    ((np.zeros((2, 2)), None), "f returned proposals (2, 2) for 3 rows of 2 parameters"),
    ((Q_OK, np.zeros(2)), "f returned qxy (2,) for 3 rows"),
    ((Q_OK, torch.zeros(4, dtype=F64)), "f returned qxy (4,) for 3 rows"),
    ((Q_OK, torch.zeros((), dtype=F64)), "f returned qxy () for 3 rows"),          # a tensor is a term, whatever it holds: one value for 3 rows
], ids=["no-pair", "triple", "Q-3x3", "Q-2x2", "qxy-2", "qxy-4", "qxy-0d-tensor"])
def test_jump_result_refuses_in_the_words_both_stages_used(r, msg):
    with pytest.raises(ValueError, match="^" + re.escape(msg) + "$"):
        stub()._jump_result(r, N, "f")


@pytest.mark.parametrize("zero", [None, 0, 0.0, np.float64(0)], ids=["None", "int", "float", "np.float64"])
def test_jump_result_takes_none_and_a_scalar_zero_as_no_term(zero):
    Q = torch.ones((N, D), dtype=F64)
    out = stub()._jump_result((Q, zero), N, "f")
    assert out[0] is Q and out[1] is None


def test_jump_result_brings_arrays_to_the_device():
    Q, qxy = stub()._jump_result([Q_OK, np.array([0.5, 0.0, -1.0])], N, "f")     # (a list is a pair too)
    assert torch.is_tensor(Q) and Q.dtype == F64 and Q.is_contiguous() and tuple(Q.shape) == (N, D) and np.array_equal(Q.numpy(), Q_OK)
    assert torch.is_tensor(qxy) and qxy.dtype == F64 and qxy.is_contiguous() and qxy.tolist() == [0.5, 0.0, -1.0]
    Q, qxy = stub()._jump_result((torch.ones((D, N), dtype=F64).t(), torch.arange(2 * N, dtype=F64)[::2]), N, "f")
    assert Q.is_contiguous() and tuple(Q.shape) == (N, D) and qxy.is_contiguous() and qxy.tolist() == [0.0, 2.0, 4.0]
    Q, qxy = stub()._jump_result((Q_OK, np.zeros((N, 1))), N, "f")                # the count is held, not the shape
    assert tuple(qxy.shape) == (N, 1)


# ---------------------------------------------------------------------- both stages use it
class Nameless(object):
    """A callable without ``__name__``: the stages then name it by its index."""

    def __init__(self, r):
        self.r = r

    def __call__(self, *a):
        return self.r


BAD = [(Q_OK,), (np.zeros((N, N)), None), (Q_OK, np.zeros(N + 1))]
BAD_MSG = ["%s must return (Q[n, ndim], qxy[n] or 0 or None)", "%s returned proposals (3, 3) for 3 rows of 2 parameters",
           "%s returned qxy (4,) for 3 rows"]


@pytest.mark.parametrize("k", range(len(BAD)))
def test_both_stages_refuse_the_same_return_value_in_the_same_words(k):
    def named(*a):
        return BAD[k]

    said = {}
    for who, func in (("named", named), ("nameless", Nameless(BAD[k]))):
        ej, ea = stub(jumps=[func]), stub(aux=[func])
        with pytest.raises(ValueError) as err_j:
            ej.jump_stage(7)
        with pytest.raises(ValueError) as err_a:
            ea.aux_stage(7)
        said[who] = (str(err_j.value), str(err_a.value))
        assert ej.lib.names() == ["ptmi_cj_work_bytes", "ptmi_cj_begin"]          # the custom stage has nothing to close
        # the auxiliary stage is closed, with nothing to put back, before the error leaves
        assert ea.lib.names() == ["ptmi_aux_begin", "ptmi_proposals", "ptmi_aux_end"] and ea.lib.calls[-1] == ("ptmi_aux_end", None, None)
    assert said["named"] == (BAD_MSG[k] % "named",) * 2
    assert said["nameless"] == (BAD_MSG[k] % "jump 0", BAD_MSG[k] % "auxiliary jump 0")


def test_jump_stage_copies_what_the_function_returned():
    seen = []

    def jump(X, it, beta):
        seen.append((tuple(X.shape), it, tuple(beta.shape)))
        return torch.ones_like(X), np.full(N, 0.5)

    e = stub(jumps=[jump])
    assert e.jump_stage(7) == N and seen == [((N, D), 7, (N,))]
    assert list(e._cj_offs) == [0, N] and e._cj_cur == 0 and e._cj_work.numel() == 0
    assert e._cj_rows.tolist() == [[1.0] * D] * N and e._cj_qxy.tolist() == [0.5] * N
    assert e.lib.calls[-1] == ("ptmi_cj_end", e._cj_work.data_ptr(), e._cj_rows.data_ptr(), e._cj_qxy.data_ptr())
    e = stub(jumps=[lambda X, it, beta: (X, 0)])                      # in place, no term: nothing to copy, no qxy pointer
    assert e.jump_stage(8) == N and e.lib.calls[-1] == ("ptmi_cj_end", e._cj_work.data_ptr(), e._cj_rows.data_ptr(), None)
    assert stub().jump_stage(9) == 0                                  # no jumps=: a no-op


def test_aux_stage_hands_the_last_result_and_term_to_the_library():
    own, term = torch.ones((N, D), dtype=F64), torch.full((N,), 0.25, dtype=F64)
    first = torch.full((N,), 2.0, dtype=F64)
    e = stub(aux=[lambda X, Q, it, beta: (Q, first), lambda X, Q, it, beta: (own, term), lambda X, Q, it, beta: (Q, None)])
    assert e.aux_stage(7) == 3
    assert e.lib.calls[-1] == ("ptmi_aux_end", own.data_ptr(), term.data_ptr())
    assert e.t["qaux"][:, 0, 0].tolist() == [2.0] * N                  # the first term was added before the second took its place
    e = stub(aux=[lambda X, Q, it, beta: (Q, None)])                  # in place, no term
    assert e.aux_stage(8) == 1 and e.lib.calls[-1] == ("ptmi_aux_end", None, None)
    assert stub().aux_stage(9) == 0 and stub().lib.calls == []        # no aux=: a no-op


def test_the_stages_behind_a_proposal_launch_run_in_their_order():
    e, order = stub(), []
    e.gradient_stage = lambda it, lg, pg: order.append(("gradient", it, lg, pg))
    e.jump_stage = lambda it: order.append(("jump", it))
    e.aux_stage = lambda it: order.append(("aux", it))
    e._proposal_stages(5, "lg", "pg")
    assert order == [("gradient", 5, "lg", "pg"), ("jump", 5), ("aux", 5)]


def test_the_built_in_callbacks_call_their_entry_points():
    e = stub()
    X = torch.zeros((5, D), dtype=F64)
    out = e.builtin_logl()(X)
    assert tuple(out.shape) == (5,) and out.dtype == F64 and e.lib.calls == [("ptmi_rows_logl", X.data_ptr(), 5, out.data_ptr())]
    out = e.builtin_logp()(X)
    assert tuple(out.shape) == (5,) and e.lib.calls[-1] == ("ptmi_rows_logp", X.data_ptr(), 5, out.data_ptr(), None)
    for make, name in ((e.builtin_logl_grad, "ptmi_rows_logl_grad"), (e.builtin_logp_grad, "ptmi_rows_logp")):
        out, g = make()(X)
        assert tuple(out.shape) == (5,) and tuple(g.shape) == (5, D) and g.dtype == F64
        assert e.lib.calls[-1] == (name, X.data_ptr(), 5, out.data_ptr(), g.data_ptr())


def test_cb_values_and_cb_grad_keep_their_own_words():
    e = stub()
    with pytest.raises(ValueError, match="^" + re.escape("logl returned 2 values for n = 3 rows") + "$"):
        e._cb_values(np.zeros(2), what="logl")
    with pytest.raises(ValueError, match="^" + re.escape("the callback returned 4 values for n = 2 rows") + "$"):
        e._cb_values(np.zeros(4), 2)
    v = torch.zeros(N, dtype=F64)
    assert tuple(e._cb_values(v).shape) == (N, 1) and e._cb_values(v).data_ptr() == v.data_ptr() and e._cb_values(v, N) is v
    with pytest.raises(ValueError, match="^" + re.escape("logl_grad must return (value[n], gradient[n, ndim])") + "$"):
        e._cb_grad(v, N, "logl_grad")
    with pytest.raises(ValueError, match="^" + re.escape("logp_grad returned value (3,) and gradient (3, 3) for 3 rows of 2 parameters: "
                                                         "expected [3] and [3, 2]") + "$"):
        e._cb_grad((v, np.zeros((N, N))), N, "logp_grad")
    g = torch.zeros((N, D), dtype=F64)
    out = e._cb_grad((v, g), N, "logl_grad")
    assert out[0] is v and out[1] is g and e._cb_grad([v, g], N, "logl_grad")[1] is g


# ---------------------------------------------------------------------- the constructor's hooks
def test_the_callback_path_refuses_ahead_of_the_other_stages():
    with pytest.raises(ValueError, match="served on the callback path") as err:
        PTEngine.with_stages(3, 2, 4, np.eye(3), aux=[print], hist=(0.0, -1.0, 4))     # two faults: aux= without split, lo > hi
    assert str(err.value) == "aux= are served on the callback path: split=True (or rows_logl=True)"


def test_the_callback_path_refuses_before_the_library_is_loaded(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded ahead of the refusal"))
    with pytest.raises(ValueError) as err:
        PTEngine(3, 2, 4, np.eye(3), jumps=[(print, 1)])
    assert str(err.value) == "jumps= are served on the callback path: split=True (or rows_logl=True)"


def test_the_checks_fill_the_cycle_and_return_w_host():
    e = PTEngine.__new__(PTEngine)
    f, g = (lambda X, it, beta: (X, None)), (lambda X, it, beta: (X, None))
    assert e._check_callback_stages(True, False, 0, (0, 0), [(f, 2), (g, 1), (f, 1)]) == 4
    assert e._jumps == [f, g] and e._fun_of_pick == [0, 0, 1, 0] and e._aux == [] and e.support_counts == (0, 0)
    assert e._check_callback_stages(False, False, 3, (0, 0), None) == 3 and e._jumps == [] and e._fun_of_pick == []
    with pytest.raises(ValueError, match="^" + re.escape("jumps= names 3 cycle entries for w_host=5") + "$"):
        e._check_callback_stages(True, False, 5, (0, 0), [(f, 3)])
    e.logl_in_support = True
    with pytest.raises(ValueError, match="logl_in_support=True is a stage of the callback path"):
        e._check_callback_stages(False, False, 0, (0, 0), None)
    assert e._check_callback_stages(False, True, 0, (0, 0), None) == 0


def test_the_attach_hook_tells_the_library_of_both_stages():
    e = stub(jumps=[engine.box_draw_jump(-1.0, 1.0), print], aux=[print])
    e._fun_of_pick = [0, 0, 1]
    e._attach_callback_stages(3)
    assert e.lib.names() == ["ptmi_cj_attach", "ptmi_aux_attach"] and e.lib.calls[0][-1] == 2
    assert tuple(e.t["cjstat"].shape) == (N, 1, 3, 2) and e.t["cjstat"].dtype == torch.int64 and not e.t["cjstat"].any()
    assert e.lib.calls[0][1].value == e.t["cjstat"].data_ptr() and [e.lib.calls[0][2][k] for k in range(3)] == [0, 0, 1]
    assert e._jumps[0].engine is e                                    # the box draw is bound to this engine
    e = stub()
    e._attach_callback_stages(0)
    assert e.lib.calls == [] and "cjstat" not in e.t
