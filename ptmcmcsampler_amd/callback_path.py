"""The callback path of ``PTEngine``: everything that serves ``split=True`` / ``rows_logl=True``.

``CallbackPath`` is a mixin of methods; ``PTEngine`` inherits from it and calls its two constructor hooks
(``_check_callback_stages`` first of all, ``_attach_callback_stages`` directly behind ``ptmi_create``).  The path reads the engine
through ``self.t``, ``self.lib``, ``self.h`` and a few scalars; the segment loop's epochs and swaps (``_epochs``, ``_segment_end``,
``swap``) stay in engine.py.  What the stages share exists once: ``_dev_f64`` (a value as a tensor the library can read),
``_jump_result`` (a batched jump's return value), ``_proposal_stages`` (what follows a proposal launch) and ``_rows_callback`` (the
built-in row kernels as callbacks).
"""
import ctypes as C

import numpy as np

from . import _lib


def _torch():
    import torch
    return torch


class _BoxDrawJump(object):
    """``PTEngine.box_draw_jump``: a batched jump whose body is ``ptmi_cj_box_draw`` (include/ptmi.h)."""
    __name__ = "boxDrawJump"

    def __init__(self, lo, hi):
        self.lo_host, self.hi_host, self.engine = np.asarray(lo, np.float64), np.asarray(hi, np.float64), None

    def bind(self, engine):
        """The engine whose stage this jump draws in (``PTEngine(jumps=...)`` binds the ones it is given): the bounds go to its GPU."""
        torch = _torch()
        self.lo = torch.as_tensor(np.array(np.broadcast_to(self.lo_host, (engine.d,))), device=engine.device)
        self.hi = torch.as_tensor(np.array(np.broadcast_to(self.hi_host, (engine.d,))), device=engine.device)
        self.engine = engine
        return self

    def __call__(self, X, iter, beta):
        eng = self.engine
        if eng is None:
            raise _lib.PtmiError("boxDrawJump runs inside PTEngine.jump_stage: give it to PTEngine(jumps=...) or PTSampler.addProposalToCycle(..., batched=True)")
        _lib.check(eng.lib.ptmi_cj_box_draw(eng.h, eng._cj_work.data_ptr(), eng._cj_cur, self.lo.data_ptr(), self.hi.data_ptr(), X.data_ptr()))
        return X, None


def box_draw_jump(lo, hi):
    """An unbound ``boxDrawJump`` (``PTEngine.box_draw_jump``) for ``PTEngine(jumps=[(box_draw_jump(lo, hi), weight), ...])``: the
    engine binds it when it is built."""
    return _BoxDrawJump(lo, hi)


class CallbackPath(object):
    """The methods of ``PTEngine`` that serve ``split=True`` / ``rows_logl=True`` (see the module docstring)."""

    # what PTEngine.with_stages sets on the instance before __init__ runs (the plain constructor leaves the class defaults)
    jumps_with_grad = False
    _aux = ()
    logl_in_support = False

    # ------------------------------------------------------------------ the constructor's hooks
    def _check_callback_stages(self, split, rows_logl, w_host, grad_weights, jumps):
        """First in ``PTEngine.__init__``, before anything is loaded or built: what ``jumps=``, ``aux=`` and ``logl_in_support`` ask
        for is checked and kept (``_jumps``, ``_fun_of_pick``, ``_aux``, ``support_counts``).  Returns ``w_host`` (``jumps=`` with
        ``w_host=0`` makes it the sum of the weights)."""
        # jumps: the w_host cycle entries as batched device callbacks (see the class docstring); fun_of_pick in cycle order, the
        # weight copies of one function sharing its index
        self._jumps, self._fun_of_pick = [], []
        if jumps is not None:
            for func, weight in jumps:
                if not callable(func) or int(weight) < 1:
                    raise ValueError("jumps=[(func, weight), ...] takes callables with weights >= 1")
                known = [k for k, f in enumerate(self._jumps) if f is func]
                if not known:
                    self._jumps.append(func)
                self._fun_of_pick += [known[0] if known else len(self._jumps) - 1] * int(weight)
            if int(w_host) == 0:
                w_host = len(self._fun_of_pick)
            if len(self._fun_of_pick) != int(w_host) or not self._jumps:
                raise ValueError("jumps= names %d cycle entries for w_host=%d" % (len(self._fun_of_pick), int(w_host)))
            if len(self._jumps) > _lib.CJ_MAXFUN:
                raise ValueError("jumps= takes at most %d different functions (got %d)" % (_lib.CJ_MAXFUN, len(self._jumps)))
            if sum(int(w) for w in grad_weights) > 0 and not self.jumps_with_grad:
                raise ValueError("custom jumps (jumps=) are mixed with gradient jumps (grad_weights) in one cycle only when asked for: "
                                 "PTEngine.with_stages(..., jumps_with_grad=True) (both stages then run behind every proposal launch)")
            if not (split or rows_logl):
                raise ValueError("jumps= are served on the callback path: split=True (or rows_logl=True)")
        elif int(w_host) > 0 and sum(int(w) for w in grad_weights) > 0:
            # (the library would hand such picks back unchanged on a split handle; only the batched stage serves them beside gradient jumps)
            raise ValueError("host-served cycle entries (w_host > 0) beside gradient jumps (grad_weights) are served as batched device "
                             "callbacks only: PTEngine.with_stages(..., jumps=[(func, weight), ...], jumps_with_grad=True)")
        # the auxiliary jumps as batched device callbacks behind every proposal launch (with_stages(aux=...); see the class docstring)
        self._aux = list(self._aux)
        if self._aux:
            if not all(callable(f) for f in self._aux):
                raise ValueError("aux=[func, ...] takes callables func(X[n, d], Q[n, d], iter, beta[n]) -> (Q[n, d], qxy[n] | 0 | None)")
            if not (split or rows_logl):
                raise ValueError("aux= are served on the callback path: split=True (or rows_logl=True)")
        # the likelihood callback only inside the prior's support (with_stages(logl_in_support=True); see the class docstring)
        self.support_counts = (0, 0)                                  # rows offered to the stage, rows it handed to logl
        if self.logl_in_support and not (split or rows_logl):
            raise ValueError("logl_in_support=True is a stage of the callback path: split=True (or rows_logl=True); the fused kernels "
                             "have no likelihood callback to spare")
        return w_host

    def _attach_callback_stages(self, w_host):
        """Directly behind ``ptmi_create``: the handle learns of the custom and the auxiliary jumps (``ptmi_cj_attach``,
        ``ptmi_aux_attach``), and the ``box_draw_jump`` entries of ``jumps=`` are bound to this engine."""
        if self._jumps:
            # proposed / accepted per pick index, by rank like jstat (get("cjstat"); device checkpoints carry it)
            torch = _torch()
            self.t["cjstat"] = torch.zeros((self.W, self.nt, int(w_host), 2), dtype=torch.int64, device=self.device)
            fop = np.ascontiguousarray(self._fun_of_pick, dtype=np.int32)
            _lib.check(self.lib.ptmi_cj_attach(self.h, C.c_void_p(self.t["cjstat"].data_ptr()), fop.ctypes.data_as(C.POINTER(C.c_int32)),
                                               len(self._jumps)))
            for f in self._jumps:
                if isinstance(f, _BoxDrawJump):
                    f.bind(self)
        if self._aux:
            _lib.check(self.lib.ptmi_aux_attach(self.h))

    def _rows_callbacks(self):
        """(logl, logp, logl_grad, logp_grad) of ``rows_logl=True``: the built-in row kernels; None where there is nothing to launch (a
        flat prior; no gradient jumps in the cycle)."""
        if getattr(self, "_rows_cb", None) is None:
            box, gj = self._par_p.size > 0, sum(self.grad_weights) > 0
            self._rows_cb = (self.builtin_logl(), self.builtin_logp() if box else None,
                             self.builtin_logl_grad() if gj else None, self.builtin_logp_grad() if gj and box else None)
        return self._rows_cb

    # ------------------------------------------------------------------ batched callbacks
    def _dev_f64(self, v):
        """``v`` as a contiguous f64 tensor on this GPU: ``v`` itself when it already is one (no copy)."""
        torch = _torch()
        if torch.is_tensor(v) and v.dtype == torch.float64 and v.device == self.device and v.is_contiguous():
            return v
        return torch.as_tensor(v, dtype=torch.float64, device=self.device).contiguous()

    def _cb_values(self, v, n=None, what="the callback"):
        """A callback's return value as a contiguous f64 tensor on this GPU (no copy when it already is one): W * nt values as [W][nt],
        or ``n`` values (the rows the support stage handed over); another count is a ValueError that names it."""
        want = self.W * self.nt if n is None else int(n)
        v = self._dev_f64(v)
        if v.numel() != want:
            raise ValueError("%s returned %d values for n = %d rows" % (what, v.numel(), want))
        return v if n is not None else v.reshape(self.W, self.nt)

    def eval_callback(self, X, logl, logp):
        """logp then logl of every row of the device tensor X [W][nt][d] through BATCHED callbacks
        ``f(X[n, d]) -> [n]`` (torch tensors on this GPU in, the same out): the device-side form of the reference's
        ``_function_wrapper`` boundary (PTMCMCSampler.py:1072-1086, called at :605-611).  Nothing is copied to the host.
        ``logp=None`` is the flat prior (no launch at all).  Where the prior is -inf the likelihood value is not used: the reference
        does not even call it (:607-608), here the accept test never reads it (ptmi_accept: -inf prior => -inf posterior).
        ``with_stages(logl_in_support=True)``: the reference's rule itself -- ``logl`` is handed only the rows whose prior is not -inf
        (``ptmi_sup_begin`` lists them in row order, one host read-back: their number ``n``): the tensor itself when that is every row
        (no copy), no call at all when it is none, else the listed rows compacted into ``rows[:n]`` (``ptmi_sup_rows``) and its ``n``
        values put back, -inf elsewhere (``ptmi_sup_end``).  A likelihood that is only defined inside the support runs that way; for a
        row-wise callback the chains are the same bit for bit.  ``support_counts`` = (rows offered, rows handed to ``logl``) so far."""
        flat = X.view(-1, self.d)
        if logp is None:
            if getattr(self, "_lp_zero", None) is None:
                self._lp_zero = _torch().zeros((self.W, self.nt), dtype=_torch().float64, device=self.device)
            lp = self._lp_zero
        else:
            lp = self._cb_values(logp(flat))
            if self.logl_in_support:
                return self._logl_in_support(flat, lp, logl), lp
        return self._cb_values(logl(flat)), lp

    def _logl_in_support(self, flat, lp, logl):
        """``eval_callback`` with the support stage: the likelihood values [W][nt] of the rows ``flat`` whose prior ``lp`` is not -inf."""
        torch = _torch()
        n_in = self.W * self.nt
        lib, h = self.lib, self.h
        if getattr(self, "_sup_work", None) is None:
            nb = C.c_size_t(0)
            _lib.check(lib.ptmi_sup_work_bytes(h, n_in, C.byref(nb)))
            self._sup_work = torch.empty(nb.value, dtype=torch.uint8, device=self.device)
            self._sup_rows = None                                     # [n_in][d], at the first partly supported batch
        work = self._sup_work.data_ptr()
        n = C.c_int64(0)
        _lib.check(lib.ptmi_sup_begin(h, work, lp.data_ptr(), n_in, C.byref(n)))
        n = int(n.value)
        self.support_counts = (self.support_counts[0] + n_in, self.support_counts[1] + n)
        if n == n_in:
            return self._cb_values(logl(flat), what="logl")           # (the stage left open is replaced by the next ptmi_sup_begin)
        out = torch.empty((self.W, self.nt), dtype=torch.float64, device=self.device)
        if n == 0:
            _lib.check(lib.ptmi_sup_end(h, work, None, out.data_ptr()))
            return out
        if self._sup_rows is None:
            self._sup_rows = torch.empty((n_in, self.d), dtype=torch.float64, device=self.device)
        _lib.check(lib.ptmi_sup_rows(h, work, flat.data_ptr(), self._sup_rows.data_ptr()))
        v = self._cb_values(logl(self._sup_rows[:n]), n, "logl (logl_in_support: of %d rows)" % n_in)
        _lib.check(lib.ptmi_sup_end(h, work, v.data_ptr(), out.data_ptr()))
        return out

    def init_state_callback(self, p0, logl, logp, i0=0):
        """init_state for a likelihood that lives in a batched callback (:479-487)."""
        torch = _torch()
        p0 = np.asarray(p0, dtype=np.float64)
        full = np.array(p0 if p0.ndim == 3 else np.broadcast_to(p0, (self.W, self.nt, self.d)))
        self.t["X"].copy_(torch.from_numpy(full))
        if self.t.get("sloc") is not None:
            self.t["sloc"].zero_()                                    # every state is in X
        ll, lp = self.eval_callback(self.t["X"], logl, logp)
        ll, lp = ll.reshape(self.W, self.nt), lp.reshape(self.W, self.nt)
        self.t["lnL"].copy_(torch.where(torch.isneginf(lp), lp, ll))               # :481-483
        self.t["lp"].copy_(lp)
        self._store_initial(i0)
        self.iter = int(i0)

    def _cb_grad(self, r, n, what):
        """A batched gradient callback's return value ``(value [n], gradient [n, d])`` as contiguous f64 tensors on this GPU (no copy
        when they already are)."""
        if not isinstance(r, (tuple, list)) or len(r) != 2:
            raise ValueError("%s must return (value[n], gradient[n, ndim])" % what)
        v, g = self._dev_f64(r[0]), self._dev_f64(r[1])
        if v.numel() != n or tuple(g.shape) != (n, self.d):
            raise ValueError("%s returned value %s and gradient %s for %d rows of %d parameters: expected [%d] and [%d, %d]"
                             % (what, tuple(v.shape), tuple(g.shape), n, self.d, n, n, self.d))
        return v, g

    def gradient_stage(self, it, logl_grad, logp_grad=None):
        """The HMC and NUTS picks of the proposals of iteration ``it`` (just made by ptmi_propose / ptmi_accept_propose): rounds of
        ``logl_grad(X[n, d]) -> (lnL[n], dlnL[n, d])`` (and ``logp_grad``, the same shape; None: a flat prior, no launch) on the rows the
        library lists (``ptmi_gj_begin`` / ``ptmi_gj_step``, include/ptmi.h), until every chain's trajectory or tree has ended: one
        round per leapfrog of the longest.  Returns the number of rounds.  A no-op without gradient jumps in the cycle."""
        if sum(self.grad_weights) <= 0:
            return 0
        if logl_grad is None:
            raise ValueError("gradient jumps are in the cycle (grad_weights=%r): the callback path needs logl_grad" % (self.grad_weights,))
        torch = _torch()
        if getattr(self, "_gj_work", None) is None:
            nb = C.c_size_t(0)
            _lib.check(self.lib.ptmi_gj_work_bytes(self.h, C.byref(nb)))
            self._gj_work = torch.empty(nb.value, dtype=torch.uint8, device=self.device)
            self._gj_rows = torch.empty((self.W * self.nt, self.d), dtype=torch.float64, device=self.device)
        lib, h, work, rows = self.lib, self.h, self._gj_work.data_ptr(), self._gj_rows
        n = C.c_int64(0)
        _lib.check(lib.ptmi_gj_begin(h, it, work, rows.data_ptr(), C.byref(n)))
        rounds = 0
        while n.value > 0:
            X = rows[:n.value]
            ll, gl = self._cb_grad(logl_grad(X), n.value, "logl_grad")
            lp = gp = None
            if logp_grad is not None:
                lp, gp = self._cb_grad(logp_grad(X), n.value, "logp_grad")
            _lib.check(lib.ptmi_gj_step(h, work, ll.data_ptr(), gl.data_ptr(), lp.data_ptr() if lp is not None else None,
                                        gp.data_ptr() if gp is not None else None, rows.data_ptr(), C.byref(n)))
            rounds += 1
        return rounds

    def _jump_result(self, r, n, what):
        """A batched jump's return value ``(Q [n, d], qxy [n] | 0 | None)`` as ``(Q, qxy)``, contiguous f64 tensors on this GPU (no
        copy when they already are); ``qxy`` is None where the jump has no term (None, or a scalar 0 that is not a tensor)."""
        if not isinstance(r, (tuple, list)) or len(r) != 2:
            raise ValueError("%s must return (Q[n, ndim], qxy[n] or 0 or None)" % what)
        Q, qxy = r
        Q = self._dev_f64(Q)
        if tuple(Q.shape) != (n, self.d):
            raise ValueError("%s returned proposals %s for %d rows of %d parameters" % (what, tuple(Q.shape), n, self.d))
        if qxy is None or (not _torch().is_tensor(qxy) and np.ndim(qxy) == 0 and qxy == 0):
            return Q, None
        qxy = self._dev_f64(qxy)
        if qxy.numel() != n:
            raise ValueError("%s returned qxy %s for %d rows" % (what, tuple(qxy.shape), n))
        return Q, qxy

    def jump_stage(self, it):
        """The custom picks of the proposals of iteration ``it`` (just made by ptmi_propose / ptmi_accept_propose) through the batched
        jumps of ``jumps=``: ``ptmi_cj_begin`` lists the chains by (function, chain slot) and copies their states out; every function
        with a non-empty span is called once, ``func(X[n, d], it, beta[n]) -> (Q[n, d], qxy[n] | 0 | None)`` on device tensors (``X``
        may be changed in place and returned); ``ptmi_cj_end`` puts the rows back as those chains' proposals with their ``qxy``.
        One host read-back (the spans' offsets); nothing else leaves the device.  Returns the number of listed chains.  A no-op
        without ``jumps=``."""
        if not self._jumps:
            return 0
        torch = _torch()
        nf, n_all = len(self._jumps), self.W * self.nt
        if getattr(self, "_cj_work", None) is None:
            nb = C.c_size_t(0)
            _lib.check(self.lib.ptmi_cj_work_bytes(self.h, C.byref(nb)))
            self._cj_work = torch.empty(nb.value, dtype=torch.uint8, device=self.device)
            self._cj_rows = torch.empty((n_all, self.d), dtype=torch.float64, device=self.device)
            self._cj_beta = torch.empty(n_all, dtype=torch.float64, device=self.device)
            self._cj_qxy = torch.empty(n_all, dtype=torch.float64, device=self.device)
            self._cj_offs = (C.c_int64 * (nf + 1))()
        lib, h, work, rows = self.lib, self.h, self._cj_work.data_ptr(), self._cj_rows
        _lib.check(lib.ptmi_cj_begin(h, it, work, rows.data_ptr(), self._cj_beta.data_ptr(), self._cj_offs))
        offs = list(self._cj_offs)
        have_qxy = []
        for f, func in enumerate(self._jumps):
            lo, hi = offs[f], offs[f + 1]
            n = hi - lo
            if n <= 0:
                continue                                              # a span of zero rows is not called
            X = rows[lo:hi]
            self._cj_cur = f                                          # (box_draw_jump: which span the library draws into)
            r = func(X, it, self._cj_beta[lo:hi])
            Q, qxy = self._jump_result(r, n, getattr(func, "__name__", "jump %d" % f))
            if Q.data_ptr() != X.data_ptr():
                X.copy_(Q)
            if qxy is None:
                continue
            self._cj_qxy[lo:hi].copy_(qxy.reshape(n))
            have_qxy.append(f)
        if have_qxy and len(have_qxy) < nf:
            for f in range(nf):
                if f not in have_qxy and offs[f + 1] > offs[f]:
                    self._cj_qxy[offs[f]:offs[f + 1]].zero_()
        _lib.check(lib.ptmi_cj_end(h, work, rows.data_ptr(), self._cj_qxy.data_ptr() if have_qxy else None))
        return offs[nf]

    def aux_stage(self, it):
        """The auxiliary jumps of ``aux=`` on the proposals of iteration ``it``, behind ``gradient_stage`` and ``jump_stage``
        (PTMCMCSampler.py:1062-1065): ``ptmi_aux_begin`` gathers every chain's state and beta, each function is called once,
        ``func(X[n, d], Q[n, d], it, beta[n]) -> (Q'[n, d], qxy[n] | 0 | None)`` with ``Q`` the proposal buffer itself or what the function
        before returned, and ``ptmi_aux_end`` puts the last ``Q'`` into the proposal buffer (nothing to copy when every function worked in
        place) and adds ``qxy``.  Several ``qxy`` are added one after the other, the reference's ``qxy += qxy_aux``.  No host read-back.
        Returns the number of functions called.  A no-op without ``aux=``."""
        if not self._aux:
            return 0
        torch = _torch()
        n = self.W * self.nt
        if getattr(self, "_aux_x", None) is None:
            self._aux_x = torch.empty((n, self.d), dtype=torch.float64, device=self.device)
            self._aux_beta = torch.empty(n, dtype=torch.float64, device=self.device)
        lib, h = self.lib, self.h
        _lib.check(lib.ptmi_aux_begin(h, it, self._aux_x.data_ptr(), self._aux_beta.data_ptr()))
        P = self.proposals().view(n, self.d)
        Q, pending = P, None
        try:
            for f, func in enumerate(self._aux):
                r = func(self._aux_x, Q, it, self._aux_beta)
                Q, qxy = self._jump_result(r, n, getattr(func, "__name__", "auxiliary jump %d" % f))
                if qxy is None:
                    continue
                if pending is not None:                               # (jump's qxy + first) + second, ...: the reference's order of additions
                    self.t["qaux"].view(n, 4)[:, 0].add_(pending.reshape(n))
                pending = qxy
        except BaseException:
            lib.ptmi_aux_end(h, None, None)                           # the stage does not stay open behind a function that raised
            raise
        _lib.check(lib.ptmi_aux_end(h, Q.data_ptr() if Q.data_ptr() != P.data_ptr() else None,
                                    pending.data_ptr() if pending is not None else None))
        return len(self._aux)

    def box_draw_jump(self, lo, hi):
        """The reference's ``UniformJump`` (tests/test_simple.py:44-62: every parameter redrawn uniformly in ``[lo, hi]``, qxy = 0)
        as a batched jump for ``jumps=``: its body is ``ptmi_cj_box_draw``, the library's own counter-based generator -- reproducible
        and independent of torch's.  Bound to this engine (the module's ``box_draw_jump`` makes an unbound one for ``PTEngine(jumps=...)``)."""
        return _BoxDrawJump(lo, hi).bind(self)

    def _proposal_stages(self, it, logl_grad, logp_grad):
        """What follows the proposal launch of iteration ``it`` ahead of the callbacks: the gradient jumps' trajectories, the custom
        jumps, then the auxiliary jumps on every jump's result (each a no-op where the cycle has no such entry)."""
        self.gradient_stage(it, logl_grad, logp_grad)
        self.jump_stage(it)
        self.aux_stage(it)

    def split_step(self, it, logl, logp, logl_grad=None, logp_grad=None):
        """One iteration of every chain with batched callbacks: ptmi_propose -> (HMC / NUTS in the cycle: the gradient stage,
        ``gradient_stage``; custom and auxiliary jumps: ``jump_stage``, ``aux_stage``) -> callbacks on the device tensor of proposals ->
        ptmi_accept.  All on the engine's stream; no host copy of the proposals."""
        if self.t["Q"] is None:
            raise _lib.PtmiError("the callback path needs the engine built with split=True")
        _lib.check(self.lib.ptmi_propose(self.h, it))
        self._proposal_stages(it, logl_grad, logp_grad)
        ll, lp = self.eval_callback(self.t["Q"], logl, logp)
        _lib.check(self.lib.ptmi_accept(self.h, it, ll.data_ptr(), lp.data_ptr()))

    def _rows_callback(self, entry, grad, *tail):
        """A built-in row kernel as a batched callback: ``f(X[n, d]) -> out[n]``, or ``(out[n], g[n, d])`` with ``grad``.  ``entry`` is
        the library's entry point ``(h, X, n, out, ...)``; the gradient's pointer follows ``out`` with ``grad``, else ``tail`` does."""
        torch = _torch()

        def rows(X):
            n = X.shape[0]
            out = torch.empty(n, dtype=torch.float64, device=X.device)
            if not grad:
                _lib.check(entry(self.h, X.data_ptr(), n, out.data_ptr(), *tail))
                return out
            g = torch.empty((n, self.d), dtype=torch.float64, device=X.device)
            _lib.check(entry(self.h, X.data_ptr(), n, out.data_ptr(), g.data_ptr()))
            return out, g

        return rows

    def builtin_logl(self):
        """The built-in isotropic or dense Gaussian as a batched CALLBACK ``f(X[n, d]) -> [n]`` (``ptmi_rows_logl``: a device kernel
        behind the C ABI, the fused kernels' bits): with it ``run_callback`` reproduces ``run`` bit for bit."""
        return self._rows_callback(self.lib.ptmi_rows_logl, False)

    def builtin_logl_grad(self):
        """... and with its gradient, ``f(X[n, d]) -> (lnL[n], dlnL[n, d])`` (``ptmi_rows_logl_grad``): the ``logl_grad`` of
        ``run_callback`` / ``gradient_stage`` for HMC and NUTS in the cycle."""
        return self._rows_callback(self.lib.ptmi_rows_logl_grad, True)

    def builtin_logp(self):
        """The built-in prior (flat or box) as a batched callback ``f(X[n, d]) -> [n]`` (``ptmi_rows_logp``)."""
        return self._rows_callback(self.lib.ptmi_rows_logp, False, None)

    def builtin_logp_grad(self):
        """... and with its gradient (zeros), ``f(X[n, d]) -> (lp[n], dlp[n, d])``."""
        return self._rows_callback(self.lib.ptmi_rows_logp, True)

    def dense_logl_callback(self, mu, P):
        """The dense Gaussian -(x - mu)^T P (x - mu) / 2 (the reference's own test likelihood, tests/test_simple.py:14-41) as a batched
        CALLBACK whose product runs on the matrix cores for the whole batch at once: (X - mu) @ P is ONE f64 GEMM of [n, d] x [d, d]
        (hipBLASLt through torch), then a row-wise dot.  The built-in ``("dense", mu, P)`` family keeps its table in LDS up to 104
        parameters; beyond, its fused kernels stream the d x d table per chain-step (6.5 s per 100 steps at 1000-d) -- this callback
        on the split path is the fast way there.  Its sums have the library's order, not the oracle's: a callback
        like a user's own, checked against NumPy."""
        torch = _torch()
        mu_t = torch.as_tensor(np.asarray(mu, dtype=np.float64), device=self.device)
        P_t = torch.as_tensor(np.ascontiguousarray(np.asarray(P, dtype=np.float64)), device=self.device)

        def logl(X):
            R = X - mu_t
            return torch.mm(R, P_t).mul_(R).sum(-1).mul_(-0.5)

        return logl

    def proposals(self):
        """The device tensor that holds the current proposals (``ptmi_proposals``): Q, or Q2 in turn after ``ptmi_accept_propose``."""
        p = C.c_void_p()
        _lib.check(self.lib.ptmi_proposals(self.h, C.byref(p)))
        q2 = self.t["Q2"]
        return q2 if q2 is not None and p.value == q2.data_ptr() else self.t["Q"]

    def callback_segment(self, it, end, logl, logp, logl_grad=None, logp_grad=None):
        """Iterations ``it .. end`` with nothing between them (no epoch, no swap: a segment of ``run``): ONE proposal launch, then per
        iteration the callbacks on the device tensor of proposals and ptmi_accept_propose -- the accept test of iteration j and the
        proposal of j + 1 in one launch, a chain's row in once and out once (csrc/ptmi_split.hip) -- and ptmi_accept behind the last.
        With HMC or NUTS in the cycle every proposal launch is followed by its gradient stage (``gradient_stage``: the batched gradient
        callbacks ``logl_grad`` / ``logp_grad``).  The same chains as ``split_step`` iteration by iteration, bit for bit."""
        if self.t["Q"] is None:
            raise _lib.PtmiError("the callback path needs the engine built with split=True")
        lib, h = self.lib, self.h
        # cycles with AM entries: the picks' increments for a piece of the segment at a time, on the matrix cores ahead of the proposals
        if getattr(self, "_am_piece", None) is None:
            v = C.c_int32(0)
            _lib.check(lib.ptmi_split_am_piece(h, C.byref(v)))
            self._am_piece = v.value
        piece = self._am_piece
        if piece:
            _lib.check(lib.ptmi_split_am_prepare(h, it, min(piece, end - it + 1)))
        _lib.check(lib.ptmi_propose(h, it))
        self._proposal_stages(it, logl_grad, logp_grad)
        for j in range(it, end):
            ll, lp = self.eval_callback(self.proposals(), logl, logp)
            if piece and (j + 1 - it) % piece == 0:                   # the proposal of j + 1 opens the next piece
                _lib.check(lib.ptmi_split_am_prepare(h, j + 1, min(piece, end - j)))
            _lib.check(lib.ptmi_accept_propose(h, j, ll.data_ptr(), lp.data_ptr()))       # (between here and ptmi_accept X is not the state: sloc)
            self._proposal_stages(j + 1, logl_grad, logp_grad)
        ll, lp = self.eval_callback(self.proposals(), logl, logp)
        _lib.check(lib.ptmi_accept(h, end, ll.data_ptr(), lp.data_ptr()))

    def callback_segment_graph(self, it, end, logl, logp):
        """``callback_segment`` as ONE hipGraph launch.  At small batches the segment is launch-bound -- two launches of a few
        microseconds per iteration, each behind a Python call -- so its launches are captured once per segment LENGTH (torch's graph
        capture on a side stream the library's stream is pointed at meanwhile; the iteration comes from a counter in device memory:
        ``ptmi_device_iter``) and replayed for every later segment of that length: set the counter, launch the graph.  The callbacks
        must be graph-safe (no host synchronisation, the same launches for every batch: any fixed torch expression or device
        kernel is).  What the captured launches bake in -- the DE ring's head, whether DE is in the cycle -- is part of the cache
        key.  Returns False where it does not apply (AM entries in the cycle: their increments are listed on the host's iteration;
        configurations the row kernels do not serve; HMC or NUTS in the cycle: their rounds are counted on the host; ``logl_in_support`` with a
        prior callback: its count is read on the host): the caller then runs
        ``callback_segment``.  Same results, bit for bit."""
        torch = _torch()
        if self.t["Q2"] is None or self.weights[1] > 0 or sum(self.grad_weights) > 0 or self._jumps or self._aux:
            return False                                              # (custom jumps: their spans are read on the host; auxiliary jumps: not captured)
        if self.logl_in_support and logp is not None:
            return False                                              # (the support stage reads its count on the host)
        if getattr(self, "_graphs", None) is None:
            self._graphs = {}
        L = end - it + 1
        key = (L, bool(self.de_on), int(self.de_head), id(logl), id(logp))
        g = self._graphs.get(key)
        lib, h = self.lib, self.h
        if g is None:
            if len(self._graphs) >= 64:               # (callbacks that are new objects at every call would capture for ever: keep the SAME callables)
                self._graphs.clear()
            # a warm-up pass of the callbacks outside the capture (lazy initialisations of the libraries behind them), then the capture
            self.eval_callback(self.t["Q"], logl, logp)
            torch.cuda.synchronize(self.device)
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(self.stream)
            g = torch.cuda.CUDAGraph()
            _lib.check(lib.ptmi_device_iter(h, 1))
            _lib.check(lib.ptmi_set_stream(h, C.c_void_p(side.cuda_stream)))
            try:
                with torch.cuda.graph(g, stream=side):
                    _lib.check(lib.ptmi_propose(h, 0))
                    for j in range(L - 1):
                        ll, lp = self.eval_callback(self.proposals(), logl, logp)
                        _lib.check(lib.ptmi_accept_propose(h, j, ll.data_ptr(), lp.data_ptr()))
                    ll, lp = self.eval_callback(self.proposals(), logl, logp)
                    _lib.check(lib.ptmi_accept(h, L - 1, ll.data_ptr(), lp.data_ptr()))
            finally:
                _lib.check(lib.ptmi_set_stream(h, C.c_void_p(self.stream.cuda_stream)))
                _lib.check(lib.ptmi_device_iter(h, 0))
            g = (g, 1 if self.proposals() is self.t["Q2"] else 0)    # ... and which buffer holds the segment's last proposals
            self._graphs[key] = g
        _lib.check(lib.ptmi_set_device_iter(h, it))
        g[0].replay()
        _lib.check(lib.ptmi_set_proposals(h, g[1]))
        return True

    def run_callback(self, niter, logl, logp, fused=True, graph=False, logl_grad=None, logp_grad=None):
        """``run`` with the likelihood and the prior in batched callbacks: the same segments (epochs and swaps between them, the
        late table of ``eig_lag`` counted in segments as ``run`` counts it in launches).  ``fused=False``: propose / accept as two
        launches per iteration (``split_step``; same results).  ``graph=True``: every segment one hipGraph launch
        (``callback_segment_graph``: for small, launch-bound batches with graph-safe callbacks; same results).  HMC in the cycle
        (``grad_weights=(0, w)``), or NUTS too (``grad_weights=(w_nuts, w_hmc)``, ``split_nuts=True``): ``logl_grad(X[n, d]) ->
        (lnL[n], dlnL[n, d])`` and ``logp_grad`` (None: a flat prior) serve their trajectories (``gradient_stage``)."""
        last = self.iter + niter
        it = self.iter + 1
        while it <= last:
            self._epochs(it)
            end = self._segment_end(it, last)
            if fused and graph and self.callback_segment_graph(it, end, logl, logp):
                pass
            elif fused:
                self.callback_segment(it, end, logl, logp, logl_grad, logp_grad)
            else:
                for j in range(it, end + 1):
                    self.split_step(j, logl, logp, logl_grad, logp_grad)
            if self.tskip > 0 and self.ntg > 1 and end % self.tskip == 0:
                self.swap(end)
            if self._eig_pending:
                self._eig_wait -= 1
                if self._eig_wait <= 0 and not (end % self.cov_update == 0 and end + 1 <= last and self.owns_cold):
                    self._eig_finish()
            it = end + 1
        self.iter = last
