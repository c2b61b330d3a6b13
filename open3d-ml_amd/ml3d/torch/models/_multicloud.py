"""What the multi-cloud inference loops share (``RandLANet.inference_many``, ``KPFCNN.inference_many``): the argument checks, the
table of clouds in flight with their concatenated device arrays, and the pinned upload of the host's per-round draws.  Nothing
here knows which model calls it: what only one model needs (its sampler calls, its per-cloud counters, KPFCNN's device copy of
the splits and its candidate buffer) stays in that model."""
import numpy as np
import torch

from ... import _abi
from ... import ops

FINISHES = ("device", "host")


def check_many_args(name, model, n_clouds, max_in_flight, seeds, draw_seeds, finish="host"):
    """The checks every ``inference_many`` starts with, messages prefixed ``name``.  Returns (max_in_flight as int, the seeds);
    ``draw_seeds(n_clouds)`` is the model's own default for ``seeds=None``."""
    _abi.require_gpu(model.device, name)
    if model.training:
        raise RuntimeError(name + ": call model.eval() first")
    if finish not in FINISHES:
        raise ValueError(name + ": finish must be 'device' or 'host'")
    S = int(max_in_flight)
    if S < 1 or S > 256:
        raise ValueError(name + ": 1 <= max_in_flight <= 256")
    if seeds is None:
        seeds = draw_seeds(n_clouds)
    if len(seeds) != n_clouds:
        raise ValueError(name + ": one seed per cloud")
    return S, seeds


def eval_labels(name, clouds, evaluate):
    """``evaluate=True``: per cloud its ground-truth labels of the FULL cloud (the dataset's label values, int32 [len(point)]) or None
    where the dict carries no ``label``; a length mismatch is a ``ValueError`` here, before any patch runs.  Otherwise all None."""
    out = [None] * len(clouds)
    if not evaluate:
        return out
    for i, c in enumerate(clouds):
        lab = c.get('label', None)
        if lab is None:
            continue
        lab = np.ascontiguousarray(np.asarray(lab).reshape(-1), dtype=np.int32)
        if lab.size != len(c['point']):
            raise ValueError("%s: cloud %d has %d points and %d labels (evaluate=True scores the FULL cloud)" % (name, i, len(c['point']), lab.size))
        out[i] = lab
    return out


def new_metric():
    """An empty ``SemSegMetric`` (imported here: ``..modules`` imports model code)."""
    from ..modules.metrics import SemSegMetric
    return SemSegMetric()


def score_on_host(result, gt, lut, num_classes):
    """Add ``'confusion'`` and ``'counts'`` of ``result['predict_labels']`` against ``gt`` to a cloud's result (None: not scored)."""
    if gt is not None:
        from ..modules.metrics import host_confusion          # (imported here, like new_metric)
        result['confusion'], result['counts'] = host_confusion(result['predict_labels'], gt, lut, num_classes)
    return result


def finish_cloud(votes, proj_inds, proj_dev=None):
    """The finish of the single-cloud loops (``inference_end``), synchronous: the float16 device ``votes`` through ``proj_inds`` by
    ``ops.vote_project`` -> ``{'predict_labels': int64, 'predict_scores': float16}``, the arrays ``np.argmax(probs, 1)[proj_inds]`` and
    ``probs[proj_inds]`` are.  ``proj_dev``: the device copy of ``proj_inds`` (int32) where the caller has one; else one upload."""
    proj = proj_dev
    if proj is None:
        proj = torch.from_numpy(np.ascontiguousarray(proj_inds, dtype=np.int32).reshape(-1)).to(votes.device)
    labels, scores = ops.vote_project(votes, proj)
    return {'predict_labels': labels.cpu().numpy().astype(np.int64), 'predict_scores': scores.cpu().numpy()}


class CloudSlots:
    """Up to ``max_in_flight`` clouds advancing in lock step.  ``slots[s]`` is the state dict of the cloud in slot s (None once
    retired with no cloud left to take its place); ``buf`` holds the concatenation over the slots of the clouds' ``points``,
    ``possibility``, ``label``, ``votes`` (float16 [n, num_classes], created here) and ``feat`` (None when the clouds carry none),
    delimited by the HOST ``splits`` [len(slots) + 1].

    ``admit()`` returns the next cloud's state -- a dict with ``n``, ``proj_inds``, the four per-point device tensors but the votes,
    ``feat`` and whatever the model counts per cloud -- or None when no cloud is left; ``retired(state, result, possibility)``
    receives a finished cloud's state, its ``{'predict_labels', 'predict_scores'}`` and its final possibilities (numpy).
    ``finish='device'``: a finished cloud's votes are projected by ``ops.vote_project`` and copied out on a copy stream, and
    ``retired`` is called from ``poll()`` -- the loop calls it where it reads back its minima -- or ``drain()`` -- before the loop
    returns -- once the copies have completed; the state may carry ``proj_dev``, the device copy of ``proj_inds`` (int32).
    ``finish='host'``: ``retired`` is called from within ``replace_finished``.
    ``evaluate``: a state that carries ``gt`` (int32 numpy [n_full], the full cloud's label values) is scored against the HOST table
    ``lut`` (``ops.label_lut``): its result gains ``'confusion'`` (int64 [C, C]) and ``'counts'`` (int64 [3]).  The labels go up once,
    at admission (``gt_dev``); ``finish='device'`` scores by ``ops.vote_confusion`` and the matrix rides the labels' staging set and
    event, ``finish='host'`` by numpy (``modules.metrics.host_confusion``).  ``return_scores=False``: ``'predict_scores'`` is None -- no score rows are
    written, staged or copied.  With both at their defaults nothing differs from a table without them."""
    ARRAYS = ('points', 'possibility', 'label', 'votes')

    def __init__(self, max_in_flight, admit, retired, device, num_classes, finish="host", evaluate=False, return_scores=True, lut=None):
        self._admit, self._retired, self.device, self.num_classes = admit, retired, device, int(num_classes)
        self.finish = finish
        self.evaluate, self.return_scores = bool(evaluate), bool(return_scores)
        self.lut = self.lut_dev = None
        if self.evaluate:
            self.lut = np.arange(self.num_classes, dtype=np.int32) if lut is None else np.ascontiguousarray(lut, dtype=np.int32)
            if finish == "device":
                self.lut_dev = torch.from_numpy(self.lut).to(device)
        self._copy = None                      # the ONE extra stream, made by the first device retire
        self._pending, self._free = [], []     # retires on their way out, oldest first; staging buffers whose copies have completed
        self.slots, self.buf, self.splits = [], {}, np.zeros(1, np.int64)
        while len(self.slots) < max_in_flight:
            st = self.admit()
            if st is None:
                break
            self.slots.append(st)
        if self.slots:
            self.rebuild()

    def admit(self):
        st = self._admit()
        if st is not None:
            st['votes'] = torch.zeros((st['n'], self.num_classes), dtype=torch.float16, device=self.device)
            if self.evaluate and self.finish == "device" and st.get('gt') is not None:
                st['gt_dev'] = torch.from_numpy(st['gt']).to(self.device)          # once per cloud, next to proj_dev
        return st

    def active(self):
        return [s_ for s_, st in enumerate(self.slots) if st is not None]

    def rows(self, slot):
        """(a, b): the rows of the cloud in ``slot`` in the concatenated arrays."""
        return int(self.splits[slot]), int(self.splits[slot + 1])

    def rebuild(self):
        """Concatenated device arrays of the clouds in the slots (one copy per array): a newly admitted cloud brings its own
        tensors, the others are views of the previous buffers.  A retired slot keeps no rows."""
        buf = self.buf
        for s_, st in enumerate(self.slots):
            if st is not None and 'points' not in st:        # lives in the old buffers
                a, b = self.rows(s_)
                st.update({name: buf[name][a:b] for name in self.ARRAYS}, feat=None if buf['feat'] is None else buf['feat'][a:b])
        live = [st for st in self.slots if st is not None]
        splits = np.zeros(len(self.slots) + 1, np.int64)
        np.cumsum([0 if st is None else st['n'] for st in self.slots], out=splits[1:])
        new = dict(feat=None)
        for name in self.ARRAYS:
            new[name] = torch.cat([st[name] for st in live]).contiguous()
        if live[0]['feat'] is not None:
            new['feat'] = torch.cat([st['feat'] for st in live]).contiguous()
        for st in live:
            for name in self.ARRAYS + ('feat',):
                st.pop(name, None)
        self.buf, self.splits = new, splits

    def retire(self, slot):
        """The ``finish='host'`` route, blocking.  Empty ``slot``: (the cloud's state, its result from its votes through its
        ``proj_inds``, its final possibilities)."""
        st = self.slots[slot]
        a, b = self.rows(slot)
        probs = self.buf['votes'][a:b].cpu().numpy()
        result = {'predict_labels': np.argmax(probs, 1)[st['proj_inds']],
                  'predict_scores': probs[st['proj_inds']] if self.return_scores else None}
        if self.evaluate:
            score_on_host(result, st.get('gt'), self.lut, self.num_classes)
        self.slots[slot] = None
        return st, result, self.buf['possibility'][a:b].cpu().numpy()

    def _staging(self, n_full, n_sub):
        """Pinned host buffers for one retire (device-to-host copies go through pinned memory, like ``PinnedUpload``'s uploads): a
        set from ``_free`` -- sets whose copies' event HAS completed, no other is ever handed out again -- or a new one.  A set has
        room for the scores only with ``return_scores`` and for a matrix and its counts only with ``evaluate``."""
        for i, sg in enumerate(self._free):
            if sg['labels'].numel() >= n_full and sg['possibility'].numel() >= n_sub:
                return self._free.pop(i)
        room = lambda n: 1 << int(max(n, 1) - 1).bit_length()
        sg = dict(labels=torch.empty(room(n_full), dtype=torch.uint8).pin_memory(),
                  possibility=torch.empty(room(n_sub), dtype=torch.float64).pin_memory())
        if self.return_scores:
            sg['scores'] = torch.empty(room(n_full) * self.num_classes, dtype=torch.float16).pin_memory()
        if self.evaluate:
            sg['eval'] = torch.empty(self.num_classes * self.num_classes + 3, dtype=torch.int64).pin_memory()
        return sg

    def retire_async(self, slot):
        """The ``finish='device'`` route.  Empty ``slot`` without stopping the loop: one ``ops.vote_project`` over the cloud's rows on
        the current stream, then the copies of labels, scores and possibilities into pinned staging on the copy stream behind an
        event.  ``poll()`` / ``drain()`` hand the result to ``retired``."""
        st = self.slots[slot]
        a, b = self.rows(slot)
        proj = st.get('proj_dev')
        if proj is None:                        # (a tree that came out of a pickle keeps host state only: one upload)
            proj = torch.from_numpy(np.ascontiguousarray(st['proj_inds'], dtype=np.int32).reshape(-1)).to(self.device)
        votes, poss = self.buf['votes'][a:b], self.buf['possibility'][a:b]
        n_full, n_sub, C_ = int(proj.numel()), b - a, self.num_classes
        gt = st.get('gt_dev') if self.evaluate else None
        ev = scores = None
        if gt is not None:                      # the matrix and its three counts in ONE tensor: one zero fill, one copy
            ev = torch.zeros(C_ * C_ + 3, dtype=torch.int64, device=self.device)
        if self.return_scores:
            labels, scores = ops.vote_project(votes, proj)
            if gt is not None:
                ops.vote_confusion(votes, proj, gt, self.lut_dev, confusion=ev[:C_ * C_].view(C_, C_), counts=ev[C_ * C_:])
        elif gt is not None:                    # labels-only evaluation: one launch
            labels = ops.vote_confusion(votes, proj, gt, self.lut_dev, confusion=ev[:C_ * C_].view(C_, C_), counts=ev[C_ * C_:], labels=True)[2]
        else:
            labels, _ = ops.vote_project(votes, proj, scores=False)
        ready = torch.cuda.Event()
        ready.record()                          # behind the projection and every round that wrote these possibilities
        if self._copy is None:
            self._copy = torch.cuda.Stream(self.device)
        sg = self._staging(n_full, n_sub)
        with torch.cuda.stream(self._copy):
            self._copy.wait_event(ready)
            sg['labels'][:n_full].copy_(labels, non_blocking=True)
            if scores is not None:
                sg['scores'][:n_full * C_].copy_(scores.reshape(-1), non_blocking=True)
            if ev is not None:
                sg['eval'].copy_(ev, non_blocking=True)
            sg['possibility'][:n_sub].copy_(poss, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self._copy)
        self.slots[slot] = None
        # rebuild() replaces the concatenated buffers right after this, and the caching allocator hands a freed block to the next
        # request of the CURRENT stream while the copy stream may still be reading it: the entry keeps ``labels``, ``scores`` and the
        # ``poss`` view (hence the old possibility buffer) referenced until ``done`` has completed, so nothing is freed early.
        # ``record_stream`` as well, for the one case in which the entry does not live that long: a loop left by an exception
        # (``on_batch`` may raise) drops the table with copies on their way.
        for src in (labels, scores, poss, ev):
            if src is not None:
                src.record_stream(self._copy)
        self._pending.append(dict(done=done, state=st, staging=sg, n_full=n_full, n_sub=n_sub, scored=ev is not None,
                                  keep=(labels, scores, poss, proj, ev, gt)))

    def _deliver(self, p):
        """``p['done']`` has completed: copy the arrays out of the staging buffers (the results OWN their memory; the buffers go
        back to ``_free``, and only now) and hand them to ``retired``."""
        sg, n_full, n_sub, C_ = p['staging'], p['n_full'], p['n_sub'], self.num_classes
        result = {'predict_labels': sg['labels'][:n_full].numpy().astype(np.int64),              # (astype copies)
                  'predict_scores': sg['scores'][:n_full * C_].numpy().reshape(n_full, C_).copy() if self.return_scores else None}
        if p['scored']:
            both = sg['eval'].numpy().copy()
            result['confusion'], result['counts'] = both[:C_ * C_].reshape(C_, C_).copy(), both[C_ * C_:].copy()
        possibility = sg['possibility'][:n_sub].numpy().copy()
        p['keep'] = None
        self._free.append(sg)
        self._retired(p['state'], result, possibility)

    def poll(self):
        """Hand over every retire whose copies have completed, oldest first, without waiting for any."""
        while self._pending and self._pending[0]['done'].query():
            self._deliver(self._pending.pop(0))

    def drain(self):
        """Wait for and hand over every retire still on its way."""
        while self._pending:
            self._pending[0]['done'].synchronize()
            self._deliver(self._pending.pop(0))

    def replace_finished(self, finished):
        """Retire the slots ``finished`` and admit the next waiting clouds into them.  True when a cloud was admitted and the
        arrays were rebuilt (one device copy per admission, not per round); otherwise the freed slots keep their rows until the
        next admission and only ``active()`` leaves them out."""
        admitted = False
        for s_ in finished:
            if self.finish == "device":
                self.retire_async(s_)
            else:
                self._retired(*self.retire(s_))
            st = self.admit()
            if st is not None:
                self.slots[s_] = st
                admitted = True
        if admitted:
            self.rebuild()
        return admitted


class PinnedUpload:
    """The host's int32 draws of a round on their way to the device: ONE pinned staging buffer and its device twin, both grown to
    the next power of two on demand, or -- ``into`` -- a given device tensor in the twin's place (the static input of a captured
    graph, never replaced).  The copy is asynchronous; the event makes it a fact that the previous upload has finished before
    the buffer is overwritten (it has, long ago).  An asynchronous copy out of PAGEABLE memory that is freed right after the
    call faulted on the MI355X ("write access to a read-only page"): host data goes up through here and nowhere else."""

    def __init__(self, device, size, into=None):
        self.device, self.fixed = device, into is not None
        self.pinned = torch.empty(int(size), dtype=torch.int32).pin_memory()
        self.dev = into if self.fixed else torch.empty(int(size), dtype=torch.int32, device=device)
        self.uploaded = torch.cuda.Event()
        self.uploaded.record()

    def stage(self, host):
        """Upload the int32 numpy array ``host`` (any shape, taken flat); returns the device view int32 [host.size]."""
        flat = torch.from_numpy(np.ascontiguousarray(host, dtype=np.int32).reshape(-1))
        n = flat.numel()
        self.uploaded.synchronize()
        if n > self.pinned.numel():
            if self.fixed:
                raise RuntimeError("PinnedUpload: %d values into a fixed device tensor of %d" % (n, self.pinned.numel()))
            size = 1 << int(n - 1).bit_length()
            self.pinned = torch.empty(size, dtype=torch.int32).pin_memory()
            self.dev = torch.empty(size, dtype=torch.int32, device=self.device)
        self.pinned[:n].copy_(flat)
        self.dev[:n].copy_(self.pinned[:n], non_blocking=True)
        self.uploaded.record()
        return self.dev[:n]
