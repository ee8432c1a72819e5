"""A deterministic audit of the stream order of `HRNet.train_forward`.

A bit comparison between the captured and the eager step may or may not lose a race on a given day.  This module needs no luck:
it keeps a vector clock per stream while the training forward runs EAGERLY and checks, for every tensor an operation reads, that
the launch which produced it happens-before the stream the reader runs on - the same stream, or a chain of `wait_stream` edges
that were issued AFTER the producer ran.  In a captured step exactly these edges become the graph's dependencies, so a missing
one is a missing dependency of the hipGraph.

Two layers:
  * `StreamClocks` / `OrderAudit`: the bookkeeping, pure Python over opaque stream keys (tests/test_stream_audit_cpu.py drives it
    with strings);
  * `audit_train_forward`: the torch side - `torch.cuda.Stream.wait_stream` wrapped at class level to log the edges, the operations
    `train_forward` is made of (the blocks' `train_forward`, `HRModule._train_row`, the transition `_train_conv_bn` calls,
    `T.fan_out_many`, `T.grad_join`, `T.fuse_sum`, `T.conv_bn_act`) wrapped to record the current stream at entry and exit.
Buffers are keyed by their storage pointer (fan-out handles are views) and kept alive for the duration, so no pointer comes back.
"""
import contextlib
from typing import Dict, Hashable, List, Optional, Tuple


class StreamClocks:
    """One vector clock per stream.  `tick(s)` = a launch on s; `wait(a, b)` = a.wait_stream(b): a learns what b knew THEN."""

    def __init__(self) -> None:
        self._vc: Dict[Hashable, Dict[Hashable, int]] = {}

    def _of(self, s) -> Dict[Hashable, int]:
        return self._vc.setdefault(s, {s: 0})

    def tick(self, s) -> Tuple[Hashable, int]:
        vc = self._of(s)
        vc[s] += 1
        return s, vc[s]

    def wait(self, waiter, waited) -> None:
        if waiter == waited:
            return
        a, b = self._of(waiter), self._of(waited)
        for k, v in b.items():
            if a.get(k, 0) < v:
                a[k] = v

    def sees(self, s, stamp: Tuple[Hashable, int]) -> bool:
        """Does a launch issued on ``s`` NOW run behind the launch ``stamp`` = (stream, clock)?"""
        return self._of(s).get(stamp[0], 0) >= stamp[1]

    def now(self, s) -> int:
        return self._of(s)[s]


class Violation:
    def __init__(self, where: str, what: str, producer, consumer, produced_at: str = "") -> None:
        self.where, self.what, self.producer, self.consumer, self.produced_at = where, what, producer, consumer, produced_at

    def __repr__(self) -> str:
        src = f" (produced at {self.produced_at})" if self.produced_at else ""
        return f"{self.where}: {self.what}: producer stream {self.producer}{src} -> consumer stream {self.consumer}, no wait in between"


class OrderAudit:
    """Producers per buffer key, consumers checked against them.  Streams and buffer keys are opaque hashables."""

    def __init__(self) -> None:
        self.clocks = StreamClocks()
        self.producer: Dict[Hashable, Tuple[Tuple[Hashable, int], str]] = {}
        self.violations: List[Violation] = []
        self.edges: List[Tuple[Hashable, Hashable]] = []       # (waiter, waited) in issue order
        self.streams_of: Dict[str, set] = {}                   # operation kind -> streams it ran on
        self.checked = 0                                       # consumer checks made against a known producer
        self.labels: Dict[Hashable, str] = {}                  # readable names of the stream keys, where the driver has any

    def wait(self, waiter, waited) -> None:
        self.edges.append((waiter, waited))
        self.clocks.wait(waiter, waited)

    def ran(self, kind: str, stream) -> None:
        self.streams_of.setdefault(kind, set()).add(stream)

    def produce(self, key, stream, where: str) -> None:
        self.producer[key] = (self.clocks.tick(stream), where)

    def consume(self, key, stream, where: str) -> bool:
        got = self.producer.get(key)
        if got is None:
            return True  # not produced by an audited operation (the network input, a parameter)
        self.checked += 1
        stamp, src = got
        if self.clocks.sees(stream, stamp):
            return True
        self.violations.append(Violation(where, "input read without an order", stamp[0], stream, src))
        return False

    def finish(self, stream, where: str = "end of train_forward") -> None:
        """The caller continues on ``stream``: it must be ordered behind the last launch of every stream that produced something."""
        last: Dict[Hashable, Tuple[int, str]] = {}
        for (s, c), src in self.producer.values():
            if c > last.get(s, (0, ""))[0]:
                last[s] = (c, src)
        for s, (c, src) in sorted(last.items(), key=lambda kv: str(kv[0])):
            if not self.clocks.sees(stream, (s, c)):
                self.violations.append(Violation(where, "stream left unjoined", s, stream, src))

    def report(self) -> str:
        return "\n".join(repr(v) for v in self.violations)


# ---- the torch side ------------------------------------------------------------------------------------------------------------------

def _tensors(obj, out: Optional[list] = None) -> list:
    """Every tensor in a nest of lists / tuples (terms of a fuse row are (tensor, scale) pairs)."""
    import torch
    out = [] if out is None else out
    if isinstance(obj, torch.Tensor):
        out.append(obj)
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            _tensors(o, out)
    return out


class _TorchAudit:
    def __init__(self, backbone, names: Dict[int, str]) -> None:
        self.core = OrderAudit()
        self.names = names
        self.keep: list = []      # every tensor seen: storage pointers stay unique while the audit runs
        self.stack: List[str] = []
        self.labels: Dict[int, str] = {}  # raw stream handle -> "main" / "side0" ...
        self.backbone = backbone

    def stream(self):
        import torch
        return torch.cuda.current_stream().cuda_stream

    def label(self, s) -> str:
        return self.labels.get(s, f"stream@{s:#x}")

    @staticmethod
    def key(t):
        return t.untyped_storage().data_ptr()

    def where(self, what: str) -> str:
        return f"{self.stack[-1]}/{what}" if self.stack else what

    def op(self, kind: str, where: str, ins, call, scope: bool = False):
        """Run ``call()`` as one audited operation reading ``ins``; its outputs that are not views of an input get a producer."""
        s0 = self.stream()
        self.core.ran(kind, s0)
        ins = _tensors(ins)
        self.keep += ins
        in_keys = set()
        for t in ins:
            if t.is_cuda:
                in_keys.add(self.key(t))
                self.core.consume(self.key(t), s0, where)
        if scope:
            self.stack.append(where)
        try:
            out = call()
        finally:
            if scope:
                self.stack.pop()
        s1 = self.stream()
        if s1 != s0:
            self.core.violations.append(Violation(where, "operation returned on another stream than it was entered on", s0, s1))
        outs = _tensors(out)
        self.keep += outs
        for t in outs:
            if t.is_cuda and self.key(t) not in in_keys:
                self.core.produce(self.key(t), s1, where)
        return out


@contextlib.contextmanager
def audit_train_forward(monkeypatch, backbone):
    """Context in which `backbone.train_forward` (an `HRNet`, called directly or through its network) runs audited; yields the
    `OrderAudit`.  Stream keys in the report are labelled main / side<i> (the branch streams of mindpose_amd.models.backbones.hrnet).
    The end-of-forward join check runs when `HRNet.train_forward` returns."""
    import torch
    from mindpose_amd.models import train_ops as T
    from mindpose_amd.models.backbones import hrnet as H

    names = {id(m): n for n, m in backbone.named_modules()}
    A = _TorchAudit(backbone, names)

    real_wait = torch.cuda.Stream.wait_stream

    def wait_stream(self, other):
        A.core.wait(self.cuda_stream, other.cuda_stream)
        return real_wait(self, other)

    monkeypatch.setattr(torch.cuda.Stream, "wait_stream", wait_stream)

    def wrap_block(cls):
        real = cls.train_forward

        def train_forward(self, x):
            return A.op("block", names.get(id(self), cls.__name__), [x], lambda: real(self, x), scope=True)
        monkeypatch.setattr(cls, "train_forward", train_forward)

    wrap_block(H.BasicBlock)
    wrap_block(H.Bottleneck)

    real_row = H.HRModule._train_row

    def _train_row(self, i, xs, handles):
        ins = [handles[j][i] for j in range(self.num_branches)]
        return A.op("row", f"{names.get(id(self), 'HRModule')}.fuse_layers.{i}", ins, lambda: real_row(self, i, xs, handles), scope=True)
    monkeypatch.setattr(H.HRModule, "_train_row", _train_row)

    real_tcb = H._train_conv_bn

    def _train_conv_bn(seq, x, relu=None):
        return A.op("conv_bn_seq", names.get(id(seq), "conv_bn"), [x], lambda: real_tcb(seq, x, relu=relu), scope=True)
    monkeypatch.setattr(H, "_train_conv_bn", _train_conv_bn)

    real_fom, real_gj, real_fs, real_cba = T.fan_out_many, T.grad_join, T.fuse_sum, T.conv_bn_act

    def fan_out_many(xs, ks):
        return A.op("fan_out_many", A.where("fan_out_many"), list(xs), lambda: real_fom(xs, ks))

    def grad_join(xs):
        return A.op("grad_join", A.where("grad_join"), list(xs), lambda: real_gj(xs))

    def fuse_sum(base, terms):
        return A.op("fuse_sum", A.where("fuse_sum"), [base, terms], lambda: real_fs(base, terms))

    def conv_bn_act(x, conv, bn, relu, res=None):
        return A.op("conv_bn_act", A.where(names.get(id(conv), "conv")), [x, res], lambda: real_cba(x, conv, bn, relu, res))

    monkeypatch.setattr(T, "fan_out_many", fan_out_many)
    monkeypatch.setattr(T, "grad_join", grad_join)
    monkeypatch.setattr(T, "fuse_sum", fuse_sum)
    monkeypatch.setattr(T, "conv_bn_act", conv_bn_act)

    real_tf = H.HRNet.train_forward

    def train_forward(self, x):
        main = A.stream()
        A.labels[main] = "main"
        out = real_tf(self, x)
        for i, st in enumerate(H._BRANCH_STREAMS.get(x.device, [])):
            A.labels.setdefault(st.cuda_stream, f"side{i}")
        cur = A.stream()
        for t in _tensors(out):
            A.core.consume(A.key(t), cur, "backbone output")
        A.core.finish(cur)
        # readable stream names in the report
        for v in A.core.violations:
            v.producer, v.consumer = A.labels.get(v.producer, v.producer), A.labels.get(v.consumer, v.consumer)
        A.core.labels = dict(A.labels)
        return out
    monkeypatch.setattr(H.HRNet, "train_forward", train_forward)

    try:
        yield A.core
    finally:
        A.keep.clear()
