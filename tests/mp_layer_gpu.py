"""The device side of the MPLayer tests: a case of tests/mp_layer_ref.py on the GPU and the C entry points of its list form."""
import contextlib
import ctypes as C

import numpy as np


class GpuLayer:
    """the case's tensors on the device and the C entry points of its list form.  case["raw_lists"]: the kernels are handed
    the padded list as it stands (dead slots point wherever the case put them) instead of the compute-side list"""

    def __init__(self, case, dev):
        import torch
        from nmrgnn_amd import _lib
        from nmrgnn_amd.graph import GraphBatch
        self.c, self.dev = case, dev
        t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        self.t = t
        N, E = case["N"], case["E"]
        atoms = np.eye(10, dtype=np.float32)[np.arange(N) % 10]
        if case["kind"] == "padded":
            gb = GraphBatch(atoms, case["nl"], case["live"].astype(np.float32), case["inv"], device=dev)
            self.nlist = gb.nlist if case.get("raw_lists") else gb.nlist_c
            self.te = t(case["e"])
        else:
            gb = GraphBatch.from_csr(atoms, case["row_ptr"], case["col"], np.ones(len(case["col"]), np.float32),
                                     inv_degree=case["inv"], device=dev)
            self.row_ptr, self.col, self.row_of = gb.row_ptr, gb.nlist, gb.row_of
            self.te = t(case["e_flat"])
        self.csc_ptr, self.csc_edge = gb.csc()
        self.th, self.tinv, self.tw = t(case["h"]), t(case["inv"]), t(case["w"])
        self.ctx = _lib.get_context(0)
        self.st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.n_ent = N * case["K"] if case["kind"] == "padded" else len(case["col"])

    def nan(self, *shape):
        import torch
        return torch.full(shape, float("nan"), device=self.dev)

    @contextlib.contextmanager
    def graph_span(self, span=None):
        """the batch's largest graph announced to the shared context (ng_ctx_set_graph_span; the case's own span by default)
        for the calls inside, and 0 = unknown again behind them"""
        lib, handle = self.ctx.lib, self.ctx.handle
        self.ctx.check(lib.ng_ctx_set_graph_span(handle, self.c["span"] if span is None else span), "span")
        try:
            yield self
        finally:
            self.ctx.check(lib.ng_ctx_set_graph_span(handle, 0), "span")

    def records(self, host=None):
        """the incoming-edge records of ng_mp_edge_records, or caller-built ones (`host` [entries, 4], mp_layer_ref.host_records)"""
        from nmrgnn_amd._lib import ptr
        c = self.c
        if host is not None:
            rec = self.nan(max(len(host), 1), 4)
            rec[:len(host)] = self.t(host)
            return rec
        rec = self.nan(c["N"] * c["K"], 4)
        self.ctx.check(self.ctx.lib.ng_mp_edge_records(self.ctx.handle, self.st, c["N"], c["K"], c["E"], ptr(self.csc_ptr),
                                                       ptr(self.csc_edge), ptr(self.te), ptr(rec)), "records")
        return rec

    def aggregate(self):
        from nmrgnn_amd._lib import ptr
        c = self.c
        A = self.nan(c["N"], c["E"], c["F"])
        if c["kind"] == "padded":
            rc = self.ctx.lib.ng_mp_aggregate(self.ctx.handle, self.st, c["N"], c["K"], c["F"], c["E"], ptr(self.th),
                                              ptr(self.nlist), ptr(self.te), ptr(A))
        else:
            rc = self.ctx.lib.ng_mp_aggregate_csr(self.ctx.handle, self.st, c["N"], c["F"], c["E"], ptr(self.th),
                                                  ptr(self.row_ptr), ptr(self.col), ptr(self.te), ptr(A))
        self.ctx.check(rc, "aggregate")
        return A

    def fwd(self, h=None, keep_A=True, w=None):
        from nmrgnn_amd._lib import ptr
        c = self.c
        N, F, E = c["N"], c["F"], c["E"]
        h_out, s, A = self.nan(N, F), self.nan(N, F), (self.nan(N, E, F) if keep_A else None)
        th = self.th if h is None else h
        tw = self.tw if w is None else w
        if c["kind"] == "padded":
            rc = self.ctx.lib.ng_mp_layer_fwd(self.ctx.handle, self.st, N, c["K"], F, E, c["act"], c["residual"], ptr(th),
                                              ptr(self.nlist), ptr(self.te), ptr(self.tinv), ptr(tw), ptr(h_out),
                                              ptr(A), ptr(s))
        else:
            rc = self.ctx.lib.ng_mp_layer_fwd_csr(self.ctx.handle, self.st, N, self.n_ent, F, E, c["act"], c["residual"],
                                                  ptr(th), ptr(self.row_ptr), ptr(self.col), ptr(self.te), ptr(self.tinv),
                                                  ptr(tw), ptr(h_out), ptr(A), ptr(s))
        self.ctx.check(rc, "fwd")
        return h_out, A, s

    def bwd(self, A, S, dH, h=None, rec=None, de_prior=None, want_dw=True, w=None):
        """dh_in, de [entries, E], dw; de accumulates onto de_prior when given; want_dw = False: dw = NULL"""
        from nmrgnn_amd._lib import ptr
        c = self.c
        N, F, E = c["N"], c["F"], c["E"]
        dh, dw = self.nan(N, F), (self.nan(F, F, E) if want_dw else None)
        de = self.nan(self.n_ent, E) if de_prior is None else de_prior.clone()
        acc = 0 if de_prior is None else 1
        th = self.th if h is None else h
        tw = self.tw if w is None else w
        if c["kind"] == "csr":
            rc = self.ctx.lib.ng_mp_layer_bwd_csr(self.ctx.handle, self.st, N, self.n_ent, F, E, c["act"], ptr(th),
                                                  ptr(self.row_ptr), ptr(self.col), ptr(self.row_of), ptr(self.te),
                                                  ptr(self.tinv), ptr(tw), ptr(A), ptr(S), ptr(self.csc_ptr),
                                                  ptr(self.csc_edge), ptr(dH), ptr(dh), ptr(de), acc, ptr(dw))
        elif rec is None:
            rc = self.ctx.lib.ng_mp_layer_bwd(self.ctx.handle, self.st, N, c["K"], F, E, c["act"], ptr(th), ptr(self.nlist),
                                              ptr(self.te), ptr(self.tinv), ptr(tw), ptr(A), ptr(S), ptr(self.csc_ptr),
                                              ptr(self.csc_edge), ptr(dH), ptr(dh), ptr(de), acc, ptr(dw))
        else:
            rc = self.ctx.lib.ng_mp_layer_bwd_rec(self.ctx.handle, self.st, N, c["K"], F, E, c["act"], ptr(th),
                                                  ptr(self.nlist), ptr(self.te), ptr(self.tinv), ptr(tw), ptr(A),
                                                  ptr(S), ptr(self.csc_ptr), ptr(self.csc_edge), ptr(dH), ptr(dh), ptr(de),
                                                  acc, ptr(dw), ptr(rec))
        self.ctx.check(rc, "bwd")
        return dh, de, dw


def de_slots(case, de):
    """de of the kernels ([entries, E]) in the padded [N, K, E] form of the reference"""
    de = de.cpu().numpy().astype(np.float64)
    if case["kind"] == "padded":
        return de.reshape(case["N"], case["K"], case["E"])
    out = np.zeros((case["N"], case["K"], case["E"]))
    out[case["rows"], case["slot"]] = de
    return out
