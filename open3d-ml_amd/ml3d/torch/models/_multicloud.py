"""What the multi-cloud inference loops share (``RandLANet.inference_many``, ``KPFCNN.inference_many``): the argument checks, the
table of clouds in flight with their concatenated device arrays, and the pinned upload of the host's per-round draws.  Nothing
here knows which model calls it: what only one model needs (its sampler calls, its per-cloud counters, KPFCNN's device copy of
the splits and its candidate buffer) stays in that model."""
import numpy as np
import torch

from ... import _abi


def check_many_args(name, model, n_clouds, max_in_flight, seeds, draw_seeds):
    """The checks every ``inference_many`` starts with, messages prefixed ``name``.  Returns (max_in_flight as int, the seeds);
    ``draw_seeds(n_clouds)`` is the model's own default for ``seeds=None``."""
    _abi.require_gpu(model.device, name)
    if model.training:
        raise RuntimeError(name + ": call model.eval() first")
    S = int(max_in_flight)
    if S < 1 or S > 256:
        raise ValueError(name + ": 1 <= max_in_flight <= 256")
    if seeds is None:
        seeds = draw_seeds(n_clouds)
    if len(seeds) != n_clouds:
        raise ValueError(name + ": one seed per cloud")
    return S, seeds


class CloudSlots:
    """Up to ``max_in_flight`` clouds advancing in lock step.  ``slots[s]`` is the state dict of the cloud in slot s (None once
    retired with no cloud left to take its place); ``buf`` holds the concatenation over the slots of the clouds' ``points``,
    ``possibility``, ``label``, ``votes`` (float16 [n, num_classes], created here) and ``feat`` (None when the clouds carry none),
    delimited by the HOST ``splits`` [len(slots) + 1].

    ``admit()`` returns the next cloud's state -- a dict with ``n``, ``proj_inds``, the four per-point device tensors but the votes,
    ``feat`` and whatever the model counts per cloud -- or None when no cloud is left; ``retired(state, result, possibility)``
    receives a finished cloud's state, its ``{'predict_labels', 'predict_scores'}`` and its final possibilities (numpy)."""
    ARRAYS = ('points', 'possibility', 'label', 'votes')

    def __init__(self, max_in_flight, admit, retired, device, num_classes):
        self._admit, self._retired, self.device, self.num_classes = admit, retired, device, int(num_classes)
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
        """Empty ``slot``: (the cloud's state, its result from its votes through its ``proj_inds``, its final possibilities)."""
        st = self.slots[slot]
        a, b = self.rows(slot)
        probs = self.buf['votes'][a:b].cpu().numpy()
        result = {'predict_labels': np.argmax(probs, 1)[st['proj_inds']], 'predict_scores': probs[st['proj_inds']]}
        self.slots[slot] = None
        return st, result, self.buf['possibility'][a:b].cpu().numpy()

    def replace_finished(self, finished):
        """Retire the slots ``finished`` and admit the next waiting clouds into them.  True when a cloud was admitted and the
        arrays were rebuilt (one device copy per admission, not per round); otherwise the freed slots keep their rows until the
        next admission and only ``active()`` leaves them out."""
        admitted = False
        for s_ in finished:
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
