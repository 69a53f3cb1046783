"""Device engine of the batched task-GP path: from flattened prior parameters theta[P, D] and a batch
of tasks to per-(task, particle) log marginal likelihoods and d(sum)/d(theta) -- the work the
reference does with a Python loop over tasks around VectorizedGP.forward / ExactGP + autograd
(meta_learn/random_gp.py:54-89,204-222; GPR_meta_mll.py:104-117).  Every arithmetic step is a HIP
kernel behind the C ABI (include/pacoh_gp.h); this file only sequences launches on the current
stream and owns the parameter layout.
"""
import os
import time
import warnings
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from . import parallel
from .util import gc_paused


def nn_param_layout(input_dim, output_dim, layer_sizes):
    """bias BEFORE weight per layer, weight row-major [out,in] (meta_learn/models.py:319-323,351-384)"""
    layout = OrderedDict()
    prev = input_dim
    for i, size in enumerate(layer_sizes):
        layout['fc_%i.bias' % (i + 1)] = size
        layout['fc_%i.weight' % (i + 1)] = size * prev
        prev = size
    layout['out.bias'] = output_dim
    layout['out.weight'] = output_dim * prev
    return layout


# covar_module kind of a ParamLayout -> its PACOH_KERNEL_* family ('NN': ARD-RBF on the learned features)
KERNEL_CODES = {'SE': L.KERNEL_RBF, 'COS': L.KERNEL_COSINE, 'M12': L.KERNEL_MATERN12, 'M32': L.KERNEL_MATERN32, 'M52': L.KERNEL_MATERN52}


class ParamLayout:
    """Flattened prior-parameter vector.  Block order follows VectorizedGP.__init__
    (meta_learn/random_gp.py:33-51): mean block, kernel_nn block, lengthscale_raw, [outputscale_raw,]
    noise_raw.  `with_outputscale` adds the ScaleKernel parameter of PACOH-MAP (GPR_meta_mll.py:218)."""

    def __init__(self, input_dim, mean_module='NN', covar_module='NN', mean_nn_layers=(32, 32),
                 kernel_nn_layers=(32, 32), feature_dim=2, with_outputscale=False):
        # 'COS': gpytorch.kernels.CosineKernel on the raw inputs (module objects only, modules.py) -- ONE raw period parameter, kept
        # in the lengthscale slot; the device sees it replicated over the input dimensions (PACOH_KERNEL_COSINE in pacoh_gp.h)
        # 'M12' | 'M32' | 'M52': gpytorch.kernels.MaternKernel(nu = 1/2, 3/2, 5/2) on the raw inputs (module objects only) -- ARD
        # lengthscales like 'SE', one raw parameter per input dimension (PACOH_KERNEL_MATERN*)
        assert mean_module in ('NN', 'constant', 'zero') and covar_module in ('NN',) + tuple(KERNEL_CODES)
        self.input_dim, self.mean_module, self.covar_module = input_dim, mean_module, covar_module
        self.kernel_code = KERNEL_CODES.get(covar_module, L.KERNEL_RBF)
        self.mean_nn_layers, self.kernel_nn_layers = tuple(mean_nn_layers), tuple(kernel_nn_layers)
        self.feature_dim = feature_dim if covar_module == 'NN' else input_dim
        self.with_outputscale = with_outputscale
        blocks = OrderedDict()
        if mean_module == 'NN':
            for k, v in nn_param_layout(input_dim, 1, mean_nn_layers).items():
                blocks['mean_nn.' + k] = v
        elif mean_module == 'constant':
            blocks['constant_mean'] = 1
        if covar_module == 'NN':
            for k, v in nn_param_layout(input_dim, feature_dim, kernel_nn_layers).items():
                blocks['kernel_nn.' + k] = v
        blocks['lengthscale_raw'] = 1 if covar_module == 'COS' else self.feature_dim
        if with_outputscale:
            blocks['outputscale_raw'] = 1
        blocks['noise_raw'] = 1
        self.blocks = blocks
        self.slices = OrderedDict()
        idx = 0
        for k, v in blocks.items():
            self.slices[k] = (idx, idx + v)
            idx += v
        self.D = idx

    def parameter_shapes(self):
        return OrderedDict((k, torch.Size((v,))) for k, v in self.blocks.items())

    def block_range(self, prefix):
        keys = [k for k in self.blocks if k.startswith(prefix)]
        if not keys:
            return None
        return self.slices[keys[0]][0], self.slices[keys[-1]][1]

    def hyper_prior_mean_std(self, weight_prior_std, bias_prior_std):
        """meta_learn/random_gp.py:126-151"""
        mean, std = torch.zeros(self.D), torch.ones(self.D)
        for name, (lo, hi) in self.slices.items():
            if name == 'noise_raw':
                mean[lo:hi] = -1.0
            elif 'mean_nn' in name or 'kernel_nn' in name:
                std[lo:hi] = weight_prior_std if 'weight' in name else bias_prior_std
        return mean, std


class TaskBatch:
    """Tasks packed for the device: x[T, n_max, d], y[T, n_max], n_valid[T] (int32); ragged tasks are
    zero padded (the kernels ignore rows >= n_valid)."""

    def __init__(self, tasks, device, dtype=torch.float32):
        sizes = [int(x.shape[0]) for x, _ in tasks]
        self.T, self.n = len(tasks), max(sizes)
        d = tasks[0][0].shape[1]
        X = np.zeros((self.T, self.n, d), dtype=np.float64)
        Y = np.zeros((self.T, self.n), dtype=np.float64)
        for t, (x, y) in enumerate(tasks):
            X[t, :sizes[t]] = x
            Y[t, :sizes[t]] = np.asarray(y).reshape(-1)
        self.sizes = np.asarray(sizes)
        self.ragged = bool((self.sizes != self.n).any())
        self.x = torch.from_numpy(X).to(dtype).to(device)
        self.y = torch.from_numpy(Y).to(dtype).to(device)
        self.n_valid = torch.from_numpy(self.sizes.astype(np.int32)).to(device)

    def select(self, idx_tensor):
        out = TaskBatch.__new__(TaskBatch)
        out.T, out.n, out.ragged = int(idx_tensor.numel()), self.n, self.ragged
        out.x, out.y, out.n_valid = L.gather_tasks(self.x, self.y, self.n_valid, idx_tensor)
        out.sizes = None
        return out


class AsyncUploader:
    """Host -> device upload of small per-step arrays (task indices, reparameterisation noise) WITHOUT stalling the host:
    a ring of pinned staging buffers, each guarded by an event, and non-blocking copies on the current stream.  A plain
    `torch.from_numpy(a).to(device)` from pageable memory blocks the host until everything queued before it has run, i.e. it
    is a stream synchronisation every step: the GPU then idles while the host issues the first launches of the next step."""

    def __init__(self, device, dtype, slots=8):
        self.device, self.dtype, self.slots = device, dtype, slots
        self.pool, self.cap, self.events, self.k = None, 0, [None] * slots, 0

    def upload(self, array):
        a = array.contiguous() if torch.is_tensor(array) else torch.from_numpy(np.ascontiguousarray(array))
        if a.numel() > self.cap:                         # (re)allocate the whole ring with ONE pinned allocation
            for ev in self.events:
                if ev is not None:
                    ev.synchronize()
            self.cap = max(a.numel(), 1)
            self.pool = torch.empty(self.slots * self.cap, dtype=self.dtype).pin_memory()
        k = self.k
        self.k = (k + 1) % self.slots
        if self.events[k] is not None:
            self.events[k].synchronize()                 # the copy that last used this slot has executed (normally long ago)
        view = self.pool[k * self.cap:k * self.cap + a.numel()].reshape(a.shape)
        view.copy_(a)                                    # (converts dtype if needed)
        out = torch.empty(a.shape, dtype=self.dtype, device=self.device)
        out.copy_(view, non_blocking=True)
        ev = self.events[k] = self.events[k] or torch.cuda.Event()
        ev.record()
        return out


def distinct_rows(idx, dtype=np.float32):
    """Each row of the task draws idx [k, tb] (with replacement) as its DISTINCT tasks: -> (rows [k, tb] int64: the row's distinct
    ids in order of first occurrence, padded with its first id; mult [k, tb]: how often each was drawn, 0 for the padding;
    n_act [k] int32: how many they are).  sum_{draws t} g(t) = sum_{j < n_act} mult[j] g(rows[j]).  A row without repeats comes back
    as it is, with all counts 1 and n_act == tb.  Vectorised over the rows: a chunk is up to 1024 rows of 1024 draws."""
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    k, tb = idx.shape
    # equal ids side by side, earlier draws first (a stable sort; 16-bit keys take numpy's radix sort: 5x faster on a full chunk)
    keys = idx.astype(np.int16) if tb > 0 and 0 <= idx.min() and idx.max() < 2 ** 15 else idx
    order = np.argsort(keys, axis=1, kind='stable')
    srt = np.take_along_axis(keys, order, axis=1)
    head = np.ones((k, tb), dtype=bool)                               # first draw of its id, in the sorted row
    head[:, 1:] = srt[:, 1:] != srt[:, :-1]
    run = np.cumsum(head, axis=1) - 1                                 # number of the id's run in the sorted row
    counts = np.bincount((run + np.arange(k)[:, None] * tb).ravel(), minlength=k * tb).reshape(k, tb)      # length of run j
    first = np.zeros((k, tb), dtype=bool)                             # ... in the row as drawn
    np.put_along_axis(first, order, head, axis=1)
    cnt_at = np.empty((k, tb), dtype=np.int64)                        # how often the id at a draw position was drawn
    np.put_along_axis(cnt_at, order, np.take_along_axis(counts, run, axis=1), axis=1)
    n_act = first.sum(axis=1).astype(np.int32)
    slot = np.cumsum(first, axis=1) - 1                               # first occurrences keep their order
    r, c = np.nonzero(first)
    rows = np.repeat(idx[:, :1], tb, axis=1)                          # (padding: the row's first id)
    mult = np.zeros((k, tb), dtype=dtype)
    rows[r, slot[r, c]] = idx[r, c]
    mult[r, slot[r, c]] = cnt_at[r, c]
    return rows, mult, n_act


class StepFeed:
    """Per-step operands of a graph-captured meta-training step (include/pacoh_gp.h, "whole steps as hipGraphs"): the task draws
    of up to `chunk` steps idx_all[chunk, tb], their step scalars sc_all[chunk, SC_COUNT] and an optional per-step payload
    aux_all[chunk, ...] (PACOH-VI: the reparameterisation noise) are uploaded with one copy each from pinned memory; select() --
    the first launch of the captured step -- moves the current row into the fixed buffers idx / sc / aux the kernels read and
    advances the device-side counter.
    dedup (set by the learner before the first upload; PACOH-SVGD on the throughput kernels): upload() rewrites every row of task
    draws as its distinct tasks with mult_all[chunk, tb] / nact_all[chunk] beside idx_all -- on the device, by one launch behind the
    copy of the raw draws (L.distinct_rows); on the host (distinct_rows, the specification) where that launch declines the shape or
    PACOH_DEDUP_HOST=1 asks for it; whoever gathers a row's tasks publishes its entries in the fixed buffers mult [tb] / nact [1]
    the step's kernels read (active())."""

    _warned_threads = False
    dedup = dedup_on_device = False

    def __init__(self, device, dtype, tb, chunk=1024, aux_shape=None):
        if not StepFeed._warned_threads:
            StepFeed._warned_threads = True
            from .util import host_cpu_budget
            if torch.get_num_threads() > host_cpu_budget():
                warnings.warn('torch uses %d intra-op CPU threads but this process may only use %d CPUs (affinity / cgroup quota): '
                              'the spinning pool can get the whole process throttled and starve the GPU of launches -- call '
                              'torch.set_num_threads(%d) or set OMP_NUM_THREADS' % (torch.get_num_threads(), host_cpu_budget(),
                                                                                  min(4, host_cpu_budget())))
        chunk = max(int(chunk), GRAPH_STEPS)              # (a several-steps graph reads GRAPH_STEPS consecutive rows)
        self.device, self.dtype, self.tb, self.chunk = device, dtype, int(tb), int(chunk)
        rows = chunk + 1                                  # (the pipelined SVGD step fetches one row ahead: pipeline())
        self.idx_all = torch.zeros(rows, tb, dtype=torch.int64, device=device) if tb > 0 else None
        self.idx = torch.zeros(tb, dtype=torch.int64, device=device) if tb > 0 else None
        self.sc_all = torch.zeros(rows, L.SC_COUNT, dtype=dtype, device=device)
        self.sc = torch.zeros(L.SC_COUNT, dtype=dtype, device=device)
        self.sc2 = self.batch = self.hyp = self._pipe = None
        self.ctr = torch.zeros(1, dtype=torch.int64, device=device)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=device)      # last-block ticket of pacoh_step_begin
        # two pinned staging sets, used alternately: the host prepares and enqueues chunk k+1 while the GPU still runs chunk k
        # (with one set it would have to wait for chunk k's upload, which sits in the stream behind chunk k-1's steps)
        self._h_idx = [torch.zeros(rows, max(tb, 1), dtype=torch.int64).pin_memory() for _ in range(2)]
        self._h_sc = [torch.zeros(rows, L.SC_COUNT, dtype=dtype).pin_memory() for _ in range(2)]
        self.aux_all = self.aux = self._h_aux = None
        if aux_shape is not None:
            self.aux_all = torch.zeros((rows,) + tuple(aux_shape), dtype=dtype, device=device)
            self.aux = torch.zeros(tuple(aux_shape), dtype=dtype, device=device)
            self._h_aux = [torch.zeros((rows,) + tuple(aux_shape), dtype=dtype).pin_memory() for _ in range(2)]
        self._ev, self._slot = [None, None], 0
        # the staging sets are FILLED through numpy views: plain memcpy on the calling thread.  torch's copy_ fans a 64 x 1024 index
        # block out over its intra-op pool (128 spinning workers on the 256-core test hosts, which have a CPU quota of 16: the
        # process was throttled for tens of milliseconds per chunk -- util.host_cpu_budget)
        self._n_idx = [t.numpy() for t in self._h_idx]
        self._n_sc = [t.numpy() for t in self._h_sc]
        self._n_aux = [t.numpy() for t in self._h_aux] if self._h_aux is not None else None
        self.mult_all = self.nact_all = self.mult = self.nact = None

    def enable_dedup(self, n_tasks=None):
        """evaluate every distinct task of a step's draw once (before the first upload).  n_tasks: the draws are task numbers below
        it -- what the device-side rewrite sizes its tables by (None: the rows are rewritten on the host)"""
        assert self.tb > 0 and self._ev[0] is None and self._ev[1] is None
        rows = self.idx_all.shape[0]
        self.dedup = True
        self.mult_all = torch.ones(rows, self.tb, dtype=self.dtype, device=self.device)
        self.nact_all = torch.full((rows,), self.tb, dtype=torch.int32, device=self.device)
        self.mult = torch.ones(self.tb, dtype=self.dtype, device=self.device)
        self.nact = torch.full((1,), self.tb, dtype=torch.int32, device=self.device)
        self._n_tasks = n_tasks
        self.dedup_on_device = n_tasks is not None and os.environ.get('PACOH_DEDUP_HOST', '0') != '1'
        self._h_mult = self._h_nact = None                # pinned staging of the host-side rewrite: _dedup_on_host

    def _dedup_on_host(self, q, idx_rows, k, kk):
        """the rewrite by distinct_rows on the host: the chunk's k rows into staging set q (rows k .. kk repeat the last one) and the
        copies of their counts; the caller copies the ids"""
        if self._h_mult is None:
            rows = self.idx_all.shape[0]
            self._h_mult = [torch.zeros(rows, self.tb, dtype=self.dtype).pin_memory() for _ in range(2)]
            self._h_nact = [torch.zeros(rows, dtype=torch.int32).pin_memory() for _ in range(2)]
        nm, nn = self._h_mult[q].numpy(), self._h_nact[q].numpy()
        self._n_idx[q][:k], hm, hn = distinct_rows(idx_rows, nm.dtype)
        nm[:k], nn[:k] = hm, hn
        nm[k:kk], nn[k:kk] = hm[k - 1], hn[k - 1]
        self.mult_all[:kk].copy_(self._h_mult[q][:kk], non_blocking=True)
        self.nact_all[:kk].copy_(self._h_nact[q][:kk], non_blocking=True)

    def active(self):
        """(nact, mult) for the kernels of a step (GPEngine.lml_and_grad(active=...)), or None"""
        return (self.nact, self.mult) if self.dedup else None

    def upload(self, idx_rows, sc_rows, aux_rows=None):
        """idx_rows: int array [k, tb]; sc_rows: k rows of L.step_scalars(); aux_rows: tensor [k, ...], k tensors [...], a callable
        (j, out_row) filling the pinned staging row of step j in place, 'device' (standard normal rows drawn by the device generator,
        no host copy), or None; resets the counter"""
        k = len(sc_rows)
        assert 0 < k <= self.chunk
        q = self._slot
        self._slot = 1 - q
        if self._ev[q] is not None:
            self._ev[q].synchronize()                    # the copies that last read this staging set have executed
        # Rows k .. GRAPH_STEPS repeat the last real row: the warm-up and capture runs of the several-steps graph read GRAPH_STEPS
        # rows whatever k is (meta_fit's first chunk is ONE step), the pipelined SVGD step one more (its update fetches the row
        # behind the one in flight), and they must see valid task indices and step scalars there -- not stale rows, not the zeros of a
        # fresh buffer (lr = 0 and bias correction 0 give NaN optimizer state)
        kk = max(k, GRAPH_STEPS) + 1
        hs = self._n_sc[q]
        hs[:k] = np.asarray(sc_rows, dtype=np.float64)
        hs[k:kk] = hs[k - 1]
        self.sc_all[:kk].copy_(self._h_sc[q][:kk], non_blocking=True)
        if self.tb > 0:
            hi = self._n_idx[q]
            idx_rows = np.asarray(idx_rows).reshape(k, self.tb)
            if self.dedup and not self.dedup_on_device:
                self._dedup_on_host(q, idx_rows, k, kk)
            else:
                hi[:k] = idx_rows
            hi[k:kk] = hi[k - 1]
            self.idx_all[:kk].copy_(self._h_idx[q][:kk], non_blocking=True)
            if self.dedup and self.dedup_on_device:
                # the raw draws are on their way: ONE launch behind the copy rewrites them in place and fills the counts
                if not L.distinct_rows(self.idx_all[:kk], self.mult_all[:kk], self.nact_all[:kk], self._n_tasks):
                    # declined (more draws per step or more tasks than its tables hold: the same for every chunk of this feed), and
                    # nothing was touched: from here on the host rewrites the rows.  This chunk's staging set is rewritten once the
                    # copy above has read it
                    self.dedup_on_device = False
                    torch.cuda.current_stream().synchronize()
                    self._dedup_on_host(q, idx_rows, k, kk)
                    hi[k:kk] = hi[k - 1]
                    self.idx_all[:kk].copy_(self._h_idx[q][:kk], non_blocking=True)
        if self.aux_all is not None:
            ha = self._n_aux[q]
            on_device = isinstance(aux_rows, str)
            if on_device:                                # 'device': standard normal rows from the device generator (PACOH-VI, noise='device')
                assert aux_rows == 'device'
                self.aux_all[:kk].normal_()
            elif callable(aux_rows):                     # aux_rows(j, out): writes step j's payload straight into the staging row
                for j in range(k):
                    aux_rows(j, self._h_aux[q][j])
            elif torch.is_tensor(aux_rows):              # (any device / dtype / requires_grad: what copy_ used to accept)
                ha[:k] = aux_rows.detach().to('cpu', self._h_aux[q].dtype).numpy().reshape(ha[:k].shape)
            else:                                        # one tensor per step
                for j, row in enumerate(aux_rows):
                    ha[j] = row.detach().to('cpu', self._h_aux[q].dtype).numpy().reshape(ha[j].shape)
            if not on_device:
                ha[k:kk] = ha[k - 1]
                self.aux_all[:kk].copy_(self._h_aux[q][:kk], non_blocking=True)
        self.ctr.fill_(-1 if self.sc2 is not None else 0)      # (pipelined step: the first forward makes it 0 -- prologue())
        self._ev[q] = self._ev[q] or torch.cuda.Event()
        self._ev[q].record()

    def pipeline(self, tasks, engine, theta):
        """switch the feed to the pipelined SVGD step (csrc/step_tail.h): persistent batch buffers, transformed hyper-parameters and
        two rows of step scalars, filled one step ahead by the update launch.  prologue() after every upload()"""
        assert self.tb > 0
        self.batch = self._empty_batch(tasks)
        self.hyper, self.hyp = self._hyper_buffers(engine, theta.shape[0], theta)
        self.sc2 = torch.zeros(2, L.SC_COUNT, dtype=self.dtype, device=self.device)
        self._row0 = torch.zeros(1, dtype=torch.int64, device=self.device)      # constant: the prologue works on row 0
        self._pipe = (tasks, theta)

    def prologue(self):
        """row 0 of the uploaded chunk into the batch buffers and sc2[0], the hyper-parameters of the particles as they are now: one
        launch, once per chunk -- not part of the step.  (upload() has left the counter at -1: the forward of the first step makes it 0)"""
        tasks, theta = self._pipe
        sc, ctr, self.sc, self.ctr = self.sc, self.ctr, self.sc2[0], self._row0     # (step_begin reads its row number from feed.ctr)
        try:
            L.step_begin(self, tasks, (self.batch.x, self.batch.y, self.batch.n_valid), theta, self.hyper, self.hyp, advance=False)
        finally:
            self.sc, self.ctr = sc, ctr

    def select(self):
        L.step_select(self.idx_all, self.sc_all, self.ctr, self.idx, self.sc, self.aux_all, self.aux)

    def _empty_batch(self, tasks):
        """the step's TaskBatch of tb tasks shaped like `tasks`, for a launch to fill (None on a rank without tasks)"""
        if self.tb == 0:
            return None
        dev, dt = tasks.x.device, tasks.x.dtype
        batch = TaskBatch.__new__(TaskBatch)
        batch.T, batch.n, batch.ragged, batch.sizes = self.tb, tasks.n, tasks.ragged, None
        batch.x = torch.empty(self.tb, tasks.n, tasks.x.shape[2], dtype=dt, device=dev)
        batch.y = torch.empty(self.tb, tasks.n, dtype=dt, device=dev)
        batch.n_valid = torch.empty(self.tb, dtype=torch.int32, device=dev) if tasks.ragged else None
        return batch

    @staticmethod
    def _hyper_buffers(engine, R, like):
        """the transformed hyper-parameters of R parameter rows through `engine` (dtype and device of `like`), for a launch to fill
        -> (the operand tuple of the transforms, (ls [R, f], outputscale [R] | None, noise [R]))"""
        off_ls, f, off_os, off_noise, _ = engine._hyper_offsets()
        dev, dt = like.device, like.dtype
        hyp = (torch.empty(R, f, dtype=dt, device=dev), torch.empty(R, dtype=dt, device=dev) if off_os >= 0 else None,
               torch.empty(R, dtype=dt, device=dev))
        return (off_ls, f, off_os, off_noise, engine.noise_floor, engine.layout.kernel_code), hyp

    def begin(self, tasks, engine=None, theta=None, advance=True, svgd=None):
        """select() + the step's task gather (+ the hyper-parameter transforms of theta through `engine`, + the SVGD distance
        matrix of svgd = (particles, workspace)) in ONE launch -> (TaskBatch | None, hypers | None); advance=False: the step's
        last launch advances the counter (L.step_begin)"""
        batch = self._empty_batch(tasks)
        out = (batch.x, batch.y, batch.n_valid) if batch is not None else None
        hyper = hyp = None
        if theta is not None and batch is not None:
            hyper, hyp = self._hyper_buffers(engine, theta.shape[0], theta)
        L.step_begin(self, tasks, out, theta if hyp is not None else None, hyper, hyp, advance=advance, svgd=svgd)
        return batch, hyp

    def begin_vi(self, tasks, engine, posterior, S):
        """begin() for a PACOH-VI step with a diagonal posterior: select (incl. the step's noise) + task gather + the step's S
        samples, their log q and transformed hyper-parameters in ONE launch -> (TaskBatch | None, hypers, theta[S, D], log_q[S])"""
        batch = self._empty_batch(tasks)
        out = (batch.x, batch.y, batch.n_valid) if batch is not None else None
        hyper, hyp = self._hyper_buffers(engine, S, posterior)
        theta = torch.empty(S, posterior.shape[1], dtype=posterior.dtype, device=posterior.device)
        log_q = torch.empty(S, dtype=posterior.dtype, device=posterior.device)
        L.step_begin_vi(self, tasks, out, posterior, theta, log_q, hyper, hyp, advance=False)
        return batch, hyp, theta, log_q


GRAPH_STEPS = 4      # steps per graph of the second graph the learners capture at world size 1 (hipGraphLaunch costs the host per
                     # launch, not per node: 0.006-0.012 ms per step with one step per graph, 0.003 with four -- what keeps the GPU fed
                     # when the host is busy with somebody else's job; tools/graph_steps_probe.py)


FIRST_CHUNK = 16     # steps in the first chunk of a call that has many more to issue (first_chunk)


def first_chunk(n_steps, chunk):
    """size of the FIRST chunk of a training call: the host prepares a chunk (task draws, step scalars, PACOH-VI's noise: 0.15 ms
    per step) before it can issue any of its steps, and while it prepares chunk k + 1 the GPU runs chunk k -- except for the first
    one, in front of which the GPU idles (meta_fit synchronises at every log line).  A small first chunk gets it started: 1.4 ms
    (SVGD, 200 steps) / 19 ms (VI, 128 steps) of idle time become 0.1 / 2.4 ms at the price of one more upload"""
    k = min(n_steps, chunk)
    if n_steps >= 4 * FIRST_CHUNK and k > FIRST_CHUNK:
        return FIRST_CHUNK
    return k


def replay_steps(n, graph_one, graph_many):
    """n steps through graph_many (GRAPH_STEPS steps per replay) and graph_one (the remainder)"""
    if graph_many is not None:
        for _ in range(n // GRAPH_STEPS):
            graph_many.replay()
        n -= (n // GRAPH_STEPS) * GRAPH_STEPS
    for _ in range(n):
        graph_one.replay()


def capture_graph(body, warmup=2, before=None):
    """hipGraph of body(): warm-up runs on a side stream first (workspaces get allocated outside the graph's pool), then the
    capture; before() (not captured) runs in front of every one of these runs -- the learners rewind their feed's step counter
    with it, so that no run reads past the rows the feed holds; the caller restores whatever state the runs changed"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            if before is not None:
                before()
            body()
    torch.cuda.current_stream().wait_stream(side)
    if before is not None:
        before()
    graph = torch.cuda.CUDAGraph()
    # several ranks: torch.distributed's watchdog thread polls events while this thread captures; with the default (global) capture
    # mode that is an error raised into the capture
    kw = {'capture_error_mode': 'thread_local'} if parallel.world()[1] > 1 else {}
    with gc_paused():                                     # (no garbage collection inside the capture: util.gc_paused)
        with torch.cuda.graph(graph, **kw):
            body()
    return graph


class StepMode:
    """Replay the captured step graph(s) or issue the same launches one by one?  Both produce identical bits.  The graph is the
    default and nearly always stays: it costs the host 0.003-0.01 ms per step (four steps per replay) against 0.1-0.2 ms for plain
    launches, so that a busy host cannot starve the GPU -- on the shared test hosts plain launches measured anywhere between 1 %
    faster than the replay (quiet host: the replay leaves a slightly larger gap between its kernel nodes on this ROCm) and 30 %
    slower (a neighbour's job on the same cores: 0.566 against 0.427 ms per cfg #3 step).  Plain launches are therefore chosen only
    when they beat the replay by 10 % in both looks' samples, which means that the replay itself is in trouble (a pathological
    graph launch).  The looks time the real training steps: a first one after PROBE steps of each kind (the first steps of a process
    are not representative: cold host, clocks ramping), a second, longer one once 4 * REPROBE more steps have run.
    PACOH_GRAPH=1 / 0 forces a mode."""
    PROBE = 6
    REPROBE = 12
    MARGIN = 0.90        # plain launches must beat the replay by 10 % (see above)

    def __init__(self):
        self.use_graph = None
        forced = os.environ.get('PACOH_GRAPH', '')
        self.forced = forced in ('0', '1')
        if self.forced:
            self.use_graph = forced == '1'
        self.timings = None
        self._since = 0
        self._looks = 0

    @staticmethod
    def _time(step, graphed, n):
        step(graphed)                                      # (not timed: first-use effects)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n - 1):
            step(graphed)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (n - 1)

    def run(self, n_steps, step, replay_many=None):
        """issue n_steps calls of step(graphed); some of them are timed to decide the mode (see the class comment).  replay_many(n)
        (optional) replays n steps with as few graph launches as the learner has graphs for (several steps per graph)"""
        done = 0
        if not self.forced:
            n = 0
            if self._looks == 0:
                n = self.PROBE
            elif self._looks == 1 and self._since >= 4 * self.REPROBE:
                n = self.REPROBE
            # the replay is timed the way it will be used: several steps per graph launch where the learner has such a graph (a
            # single-step replay pays the launch of the graph once per step -- on a slow host that alone decided for plain launches)
            ng = n if replay_many is None else -(-n // GRAPH_STEPS) * GRAPH_STEPS
            cost = 2 * (n + ng + (GRAPH_STEPS if replay_many is not None else 0))
            if n and n_steps >= max(cost, 5 * n):
                def graph_time():
                    if replay_many is None:
                        return self._time(step, True, ng)
                    replay_many(GRAPH_STEPS)               # (not timed: first-use effects)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    replay_many(ng)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) / ng
                # (each kind twice, interleaved, the faster sample counts: one hiccup of the host or the clocks during a handful of
                #  steps must not decide the mode for the rest of the run)
                t = [min(pair) for pair in zip(*[[self._time(step, False, n), graph_time()] for _ in range(2)])]
                self.timings = {'eager_ms': t[0] * 1e3, 'graph_ms': t[1] * 1e3, 'steps_each': n}
                self.use_graph = not (t[0] < self.MARGIN * t[1])
                # one decision for all ranks: with the collective captured in the step graph a rank that replays while a peer issues
                # eagerly still matches call for call, but the run would no longer be reproducible per rank -- and with
                # torch.distributed between two graphs the two modes must not mix at all.  Graph mode wins unless every rank prefers
                # plain launches.
                from . import parallel
                if parallel.world()[1] > 1:
                    self.use_graph = not parallel.agree_all(not self.use_graph)
                self._looks += 1
                done = cost
        graphed = True if self.use_graph is None else self.use_graph
        if graphed and replay_many is not None:
            replay_many(n_steps - done)
        else:
            for _ in range(n_steps - done):
                step(graphed)
        self._since += n_steps


class StepDriver:
    """The training loop the meta-learners share: their steps are drawn and uploaded in chunks (StepFeed), captured once as
    hipGraphs and replayed, or issued launch by launch (StepMode decides; both give the same bits).  A learner provides
    _setup_step(tb_local) (its buffers: _new_step), _body_likelihood / _body_update (the launches before and after the step's one
    all-reduce, _exchange), _step_scalars (the rows L.step_scalar_rows makes for a chunk's task draws), and where it differs from
    the defaults below: the chunk sizes, the per-step payload of the feed, the work of a chunk"""
    GRAPH_CHUNK = 1024
    _STEP_STATE = ()             # names of the learner's tensors a step changes (parameters, optimizer state): restored after a capture
    _feed = _graphs = _graph_many = None
    _pipelined = False

    # ---- the step's buffers -------------------------------------------------------------------------------------------------------
    def _local_batch_size(self):
        rank, world = parallel.world()
        return len(range(rank, self.task_batch_size, world))          # (= len(parallel.shard(range(B))), without the array)

    def _new_step(self, tb_local, rows, chunk, aux_shape=None):
        """what every step holds: ONE all-reduce operand _packed = gradient [rows, D] | likelihood sums [rows] (zeroed), the Cholesky
        failure flag, the feed of tb_local tasks per step; no graphs yet -> (gradient view, sums view)"""
        self._packed, grad, sums = parallel.packed_score_buffer(rows, self.layout.D, self.dtype, self.device)
        self._packed.zero_()
        self._fail = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._feed = StepFeed(self.device, self.dtype, tb_local, chunk=chunk, aux_shape=aux_shape)
        self._graphs = self._graph_many = None
        return grad, sums

    def _exchange(self):
        parallel.all_reduce_buffer_(self._packed)         # ONE exchange per step, in place

    # ---- the task draws of a chunk ----------------------------------------------------------------------------------------------
    def _take_idx(self, k):
        """the next k global task draws, int64 [k, B]: with replacement (the reference's rds_numpy.choice / randint per iteration);
        one randint call of shape [k, B] consumes the numpy stream exactly like k calls of size B"""
        return self.rds_numpy.randint(0, self.tasks.T, size=(k, self.task_batch_size))

    def _draw_steps(self, k):
        """this rank's shard of the next k steps' task draws (None where it has no tasks) and the steps' scalar rows"""
        idx = self._take_idx(k)
        sc_rows = self._step_scalars(idx)
        rank, world = parallel.world()
        local = np.ascontiguousarray(idx[:, rank::world])
        parallel.check_same_draws(local, sc_rows)
        return (local if local.shape[1] > 0 else None), sc_rows

    def _step_payload(self):
        """the feed's per-step payload of the next chunk (StepFeed.upload's aux_rows)"""
        return None

    def _chunk_size(self, n_steps, last):
        """steps in the next chunk of a training call with n_steps left; last: the previous chunk's size (0: the call's first)"""
        return first_chunk(n_steps, self._feed.chunk) if last == 0 else min(n_steps, self._feed.chunk)

    # ---- graphs and steps -------------------------------------------------------------------------------------------------------
    def _graphs_allowed(self):
        # (large contexts run the HBM-resident path, whose launch sequence sets kernel attributes: keep it eager)
        return (os.environ.get('PACOH_NO_GRAPH', '0') != '1' and self.tasks.n <= L.gp_small_max_n(self.dtype, True)
                and not L.FORCE_DENSE)

    def _prologue(self):
        """once per uploaded chunk, outside the step: the pipelined step's first row and hyper-parameters"""
        if self._pipelined:
            self._feed.prologue()

    def _build_graphs(self):
        """the hipGraphs of one step = _body_likelihood -> _exchange -> _body_update: ((whole step,), four steps) when the exchange
        can be captured (world size 1, or RCCL on the compute stream: parallel.collective_in_graph()), else ((likelihood, update),
        None) around the eager torch.distributed call.  Captured with real operands in the feed; the state the warm-up and capture
        runs change is restored"""
        feed = self._feed
        state = [getattr(self, name) for name in self._STEP_STATE] + [feed.ctr, self._fail]
        saved = [t.clone() for t in state]

        def rewind():
            if feed.sc2 is not None:
                feed.ctr.fill_(-1)                        # pipelined step: row 0 fetched again, counter = -1
                feed.prologue()
            else:
                feed.ctr.zero_()
        if parallel.collective_in_graph():
            def whole():
                self._body_likelihood()
                self._exchange()
                self._body_update()

            def several():
                for _ in range(GRAPH_STEPS):
                    whole()
            # (the large-context path allocates O(tasks x n^2) scratch per step inside the graph's pool: one step per graph there)
            self._graphs = (capture_graph(whole, before=rewind),)
            self._graph_many = capture_graph(several, before=rewind) if self.tasks.n <= 128 else None
        else:
            self._graphs = (capture_graph(self._body_likelihood, before=rewind), capture_graph(self._body_update, before=rewind))
            self._graph_many = None
        for t, sv in zip(state, saved):
            t.copy_(sv)
        self._prologue()                                  # (of the restored state)

    def _run_step(self, graphed):
        """one step: replayed from the captured graphs, or the same launches issued one by one"""
        if graphed:
            self._graphs[0].replay()
            if len(self._graphs) > 1:
                self._exchange()
                self._graphs[1].replay()
        else:
            with L.roctx_range('likelihood'):              # (no-ops unless PACOH_ROCTX=1)
                self._body_likelihood()
            with L.roctx_range('exchange'):
                self._exchange()
            with L.roctx_range('update'):
                self._body_update()

    def _run_chunk(self, k, graphed):
        """the uploaded chunk's k steps"""
        self._prologue()
        if graphed and self._graphs is None:
            self._build_graphs()
        if graphed:
            # replay or eager launches, whichever is faster here (StepMode); several steps per replay where possible
            many = (lambda n: replay_steps(n, self._graphs[0], self._graph_many)) if len(self._graphs) == 1 else None
            self._step_mode.run(k, self._run_step, many)
        else:
            for _ in range(k):
                self._run_step(False)

    def _train_steps(self, n_steps):
        """the next n_steps steps of the training loop (task draws from rds_numpy, learning rates from the scheduler), in chunks:
        the host draws and uploads chunk k + 1 while the GPU runs chunk k"""
        self._setup_step(self._local_batch_size())
        graphed = self._graphs_allowed()
        k = 0
        while n_steps > 0:
            k = self._chunk_size(n_steps, k)
            idx_rows, sc_rows = self._draw_steps(k)
            self._feed.upload(idx_rows, sc_rows, self._step_payload())
            self._run_chunk(k, graphed)
            self.opt_step += k
            for _ in range(k):
                self.lr_scheduler.step()
            n_steps -= k

    # ---- meta_fit ---------------------------------------------------------------------------------------------------------------
    def _check_numerics(self):
        """raise where the reference raises: gpytorch's psd_safe_cholesky -> NotPSDError (read at synchronisation points only)"""
        flag = getattr(self, '_fail', None)
        bad = flag is not None and int(flag.item()) != 0
        # the all-reduced sums that turn non-finite when another rank's Cholesky failed: SVGD's / VI's likelihood sums, MAP's loss
        reduced = getattr(self, '_lik', None)
        if reduced is None:
            reduced = getattr(self, '_g_loss', None)
        if not bad and parallel.world()[1] > 1 and reduced is not None:
            # another rank's shard failed: its NaN likelihood sums reach every rank through the all-reduce, so that all ranks raise
            # at the same synchronisation point (a rank raising alone would leave the others waiting in the next collective)
            bad = not bool(torch.isfinite(reduced).all())
        if bad:
            if flag is not None:
                flag.zero_()
            raise NotPSDError('a task kernel matrix was not positive definite even after adding jitter (1e-6 .. 1e-4)')

    def _fit_loop(self, n_iter, log_period, valid_tuples, verbose, run, loss=None):
        """meta_fit's iterations (GPR_meta_*.py): run(n) performs the next n; a line is logged after the first one and then every
        log_period -- with loss(itr) if given and the validation metrics of valid_tuples if given -> n_iter"""
        if n_iter is None:
            n_iter = self.num_iter_fit
        t = time.time()
        itr = 0
        while itr < n_iter:
            nxt = 1 if itr == 0 else min(n_iter, (itr // log_period + 1) * log_period)      # up to the next log line
            run(nxt - itr)
            itr = nxt
            if itr == 1 or itr % log_period == 0:
                torch.cuda.synchronize()
                duration = time.time() - t
                message = 'Iter %d/%d' % (itr, self.num_iter_fit)
                if loss is not None:
                    message += ' - Loss: %.6f' % loss(itr)
                message += ' - Time %.2f sec' % duration
                self._check_numerics()
                t = time.time()
                if valid_tuples is not None:
                    valid_ll, valid_rmse, calibr_err = self.eval_datasets(valid_tuples)
                    message += ' - Valid-LL: %.3f - Valid-RMSE: %.3f - Calib-Err %.3f' % (valid_ll, valid_rmse, calibr_err)
                self._last_log = message
                if verbose:
                    self.logger.info(message)
        return n_iter


class NotPSDError(RuntimeError):
    """a task's kernel matrix was not positive definite even with the jitter ladder -- what gpytorch's psd_safe_cholesky raises
    (gpytorch.utils.errors.NotPSDError) inside the reference's loss evaluation"""


class GPEngine:
    """Sequences the kernels of one LML(+grad) evaluation for all (task, particle) pairs."""

    def __init__(self, layout, noise_floor=0.0):
        self.layout = layout
        self.noise_floor = float(noise_floor)
        self._ws = {}

    # -- pieces -----------------------------------------------------------------------------------
    def _hyper_offsets(self):
        lay = self.layout
        off_os = lay.slices['outputscale_raw'][0] if lay.with_outputscale else -1
        off_c = lay.slices['constant_mean'][0] if lay.mean_module == 'constant' else -1
        return lay.slices['lengthscale_raw'][0], lay.feature_dim, off_os, lay.slices['noise_raw'][0], off_c

    def _hypers(self, theta):
        off_ls, f, off_os, off_noise, _ = self._hyper_offsets()
        return L.hyper_fwd(theta, off_ls, f, off_os, off_noise, self.noise_floor, kernel=self.layout.kernel_code)

    def _paired_nets(self):
        """both networks present with the same hidden shape -> (mean block offset, kernel block offset), else None"""
        lay = self.layout
        if lay.mean_module == 'NN' and lay.covar_module == 'NN' and lay.mean_nn_layers == lay.kernel_nn_layers:
            return lay.block_range('mean_nn.')[0], lay.block_range('kernel_nn.')[0]
        return None

    FWD_GP_MIN_PROBLEMS = 4096   # one resident round of the GP kernel: from there on the separate forward launch pays for a nearly
                                 # empty last round of workgroups (profiles/fwd_gp_bench.txt)

    def _use_fwd_gp(self, B, P, n, outputscale, dtype):
        """lml_and_grad runs the two networks' forward inside the GP launch (L.fwd_gp_lml_fwdbwd): fp32, RBF without outputscale, paired
        fused networks of 1-2 hidden layers, d_in <= 4, f <= 2, n == 64 -- from FWD_GP_MIN_PROBLEMS (task, parameter row) problems.
        PACOH_FWD_GP=0 / 1: never / wherever eligible (tests, A/B)"""
        force = os.environ.get('PACOH_FWD_GP')
        lay = self.layout
        if force == '0' or self._paired_nets() is None or (force != '1' and B < self.FWD_GP_MIN_PROBLEMS):
            return False
        return L.fwd_gp_applicable(B, P, n, P, lay.input_dim, list(lay.mean_nn_layers), lay.feature_dim, outputscale is not None,
                                   L.MEAN_VECTOR, dtype, kernel=lay.kernel_code)

    def _features(self, theta, x, T, n, theta_per_task=False, keep=False, svgd_tail=None, active=None):
        """kernel inputs z (+ divisor) and mean (+ mode) for B = T*P problems (b = t*P + p: task t, parameter row p).
        theta_per_task: theta holds T*S rows, S of its own per task -- the same kernels with P = T*S parameter rows, ONE
        problem per row (B = T*S) and inputs shared by S consecutive problems.  keep: park the activations the backward of the
        SAME step needs in self._ws['stash'] (lml_and_grad)"""
        lay = self.layout
        P, D = theta.shape
        B, x_div = (P, P // T) if theta_per_task else (T * P, P)
        pair = self._paired_nets()
        if pair is not None:                               # mean + kernel-feature network in one call (one launch on the fused path)
            stash = None
            if keep:
                key = ('stash', B, n)                      # one stash per batch shape: a captured graph keeps using its own
                stash = self._ws[key] = L.mlp2_stash(x, P, lay.input_dim, list(lay.mean_nn_layers), 1, lay.feature_dim, B, n,
                                                     self._ws.get(key))
            mean, z = L.mlp2_fwd(x, x_div, theta, P, lay.input_dim, list(lay.mean_nn_layers), pair[0], 1, pair[1],
                                 lay.feature_dim, B, n, ws_holder=self._ws, stash=stash,
                                 svgd_tail=svgd_tail[:3] if svgd_tail is not None else None, active=active)
            return z, 1, mean.reshape(B, n), L.MEAN_VECTOR
        assert active is None, 'distinct-task steps run on the paired fused networks only'
        if svgd_tail is not None:
            L.svgd_dist_advance(*svgd_tail[:3])            # (no paired forward launch to ride in)
        one_net = (lay.covar_module == 'NN') != (lay.mean_module == 'NN')      # the backward of ONE network can read a stash too
        if lay.covar_module == 'NN':
            lo, _ = lay.block_range('kernel_nn.')
            stash = None
            if keep and one_net:
                stash = self._ws[('stash1', B, n)] = L.mlp_stash(x, P, lay.input_dim, list(lay.kernel_nn_layers), lay.feature_dim, B, n,
                                                                 self._ws.get(('stash1', B, n)))
            z = L.mlp_fwd(x, x_div, theta[:, lo:], D, P, lay.input_dim, list(lay.kernel_nn_layers), lay.feature_dim, B, n,
                          ws_holder=self._ws, stash=stash)
            z_div = 1
        else:
            z, z_div = x, x_div
        if lay.mean_module == 'NN':
            lo, _ = lay.block_range('mean_nn.')
            stash = None
            if keep and one_net:
                stash = self._ws[('stash1', B, n)] = L.mlp_stash(x, P, lay.input_dim, list(lay.mean_nn_layers), 1, B, n,
                                                                 self._ws.get(('stash1', B, n)))
            mean = L.mlp_fwd(x, x_div, theta[:, lo:], D, P, lay.input_dim, list(lay.mean_nn_layers), 1, B, n,
                             ws_holder=self._ws, stash=stash).reshape(B, n)
            mode = L.MEAN_VECTOR
        elif lay.mean_module == 'constant':
            lo, hi = lay.slices['constant_mean']
            mean, mode = theta[:, lo:hi].contiguous().reshape(-1), L.MEAN_CONST
        else:
            mean, mode = None, L.MEAN_ZERO
        return z, z_div, mean, mode

    # -- public -----------------------------------------------------------------------------------
    def lml(self, theta, batch):
        """per-datapoint LML of every (task, particle): [T, P] (no gradients)"""
        P = theta.shape[0]
        T, n = batch.T, batch.n
        ls, os_, noise = self._hypers(theta)
        z, z_div, mean, mode = self._features(theta, batch.x, T, n)
        lml, _, _, info = L.gp_lml_fwd(z, z_div, mean, mode, batch.y, P, ls, os_, noise, T * P, P,
                                       n_valid=batch.n_valid if batch.ragged else None, kernel=self.layout.kernel_code)
        return lml.reshape(T, P), info

    def lml_and_grad(self, theta, batch, weight=1.0, lik_out=None, lik_scale=1.0, grad_out=None, fail_flag=None, hypers=None,
                     svgd_tail=None, opt=None, active=None):
        """returns (lml[T,P], grad[P,D]) with grad = d(weight * sum_t lml[t,p]) / d theta[p];
        lik_out[P] (optional) receives lik_scale * sum_t lml[t,p] from the same launch that reduces the hyper-gradients;
        grad_out[P,D] (optional, contiguous) is used for the gradient instead of a fresh tensor;
        fail_flag (optional int32[1]) is raised by that launch if any problem's Cholesky failed even with jitter;
        svgd_tail = (particles, workspace, counter, want_bandwidth): the pipelined SVGD step's distance matrix and counter
        increment, in extra workgroups of the forward launch where there is one (L.mlp2_fwd), and -- want_bandwidth -- its median
        bandwidth by one more workgroup of the hyper-parameter reduction (L.hyper_bwd);
        opt (L.adam_inline(...), one parameter row): the AdamW step is applied to every gradient entry where it is finished;
        active = (n_act int32 [1], task_w [T]) in device memory (StepFeed.active()): the batch holds the DISTINCT tasks of a draw
        with replacement in its first n_act slots and task_w their multiplicities -- only those are evaluated, each counting
        task_w times: grad = d(weight * sum_t task_w[t] lml[t,p]) / d theta[p]; the rows of the returned lml behind n_act are
        undefined.  fp32, paired fused networks, n <= 128, f <= 4 only."""
        lay = self.layout
        P, D = theta.shape
        T, n = batch.T, batch.n
        B = T * P
        dev, dt = theta.device, theta.dtype
        ls, os_, noise = hypers if hypers is not None else self._hypers(theta)      # (hypers: already transformed by pacoh_step_begin)
        fwd_gp = self._use_fwd_gp(B, P, n, os_, dt)
        if not fwd_gp:
            z, z_div, mean, mode = self._features(theta, batch.x, T, n, keep=True, svgd_tail=svgd_tail, active=active)
        g = None                                        # weight 1: the kernels take g_lml = NULL
        if float(weight) != 1.0:
            gkey = ('g', B, dt, dev)                    # ONE upstream-gradient vector per batch shape, refilled when the weight changes
            ent = self._ws.get(gkey)
            if ent is None or ent[1] != float(weight):
                g = ent[0] if ent is not None else torch.empty(B, dtype=dt, device=dev)
                g.fill_(float(weight))
                ent = self._ws[gkey] = (g, float(weight))
            g = ent[0]
        if fwd_gp:
            # the two networks' forward runs inside the GP launch (csrc/gp_fwd_reg.hip): one launch less, z / mean stay on the chip
            pair = self._paired_nets()
            key = ('stash', B, n)                          # (as _features(keep=True): the backward below reads it)
            stash = self._ws[key] = L.mlp2_stash(batch.x, P, lay.input_dim, list(lay.mean_nn_layers), 1, lay.feature_dim, B, n,
                                                 self._ws.get(key))
            lml, d_z, d_mean, d_ls, d_os, d_noise, info = L.fwd_gp_lml_fwdbwd(
                batch.x, P, theta, P, lay.input_dim, list(lay.mean_nn_layers), pair[0], pair[1], lay.feature_dim, batch.y, P, ls, noise,
                B, n, n_valid=batch.n_valid if batch.ragged else None, g_lml=g, stash=stash,
                svgd_tail=svgd_tail[:3] if svgd_tail is not None else None, active=active)
        else:
            lml, d_z, d_mean, d_ls, d_os, d_noise, info = L.gp_lml_fwdbwd(
                z, z_div, mean, mode, batch.y, P, ls, os_, noise, B, P,
                n_valid=batch.n_valid if batch.ragged else None, g_lml=g, want_dz=(lay.covar_module == 'NN'), kernel=lay.kernel_code,
                active=active)
        grad = grad_out if grad_out is not None else torch.empty(P, D, dtype=dt, device=dev)   # every block is written below
        pair = self._paired_nets()
        off_ls, f, off_os, off_noise, off_c = self._hyper_offsets()
        hyper = dict(lml=lml if lik_out is not None else None, lik=lik_out, lik_scale=lik_scale,
                     info=info if fail_flag is not None else None, fail_flag=fail_flag)
        if svgd_tail is not None and svgd_tail[3]:
            hyper['svgd_bw'] = (svgd_tail[1],) + tuple(svgd_tail[0].shape)
        if opt is not None:                                 # PACOH-MAP at world size 1: the AdamW step rides in the gradient epilogue
            hyper['opt'] = opt
        if pair is not None:
            # both networks' backward + the hyper-parameter reduction (softplus chain rule, likelihood sums, failure flag): one call,
            # on the fused path two launches
            self._ws['mk'] = L.mlp2_bwd_hyper(batch.x, P, theta, P, lay.input_dim, list(lay.mean_nn_layers), pair[0], 1,
                                              d_mean.reshape(B, n, 1), pair[1], lay.feature_dim, d_z, grad, B, n, T, off_ls, f, off_os,
                                              off_noise, off_c, d_ls, d_os, d_noise, None, workspace=self._ws.get('mk'),
                                              stash=self._ws.get(('stash', B, n)), active=active, **hyper)
            return lml.reshape(T, P), grad, info
        assert active is None
        d_const = d_mean if lay.mean_module == 'constant' else None
        if (lay.covar_module == 'NN') != (lay.mean_module == 'NN'):
            # ONE network: its backward and the hyper-parameter reduction in one call (one launch less on the fused path)
            if lay.covar_module == 'NN':
                (lo, _), layers, d_out, g_net = lay.block_range('kernel_nn.'), lay.kernel_nn_layers, lay.feature_dim, d_z
            else:
                (lo, _), layers, d_out, g_net = lay.block_range('mean_nn.'), lay.mean_nn_layers, 1, d_mean.reshape(B, n, 1)
            self._ws['k1'] = L.mlp_bwd_hyper(batch.x, P, theta, lo, P, lay.input_dim, list(layers), d_out, g_net, grad, B, n, T, off_ls, f,
                                             off_os, off_noise, off_c, d_ls, d_os, d_noise, d_const, kernel=lay.kernel_code,
                                             workspace=self._ws.get('k1'), stash=self._ws.get(('stash1', B, n)), **hyper)
            return lml.reshape(T, P), grad, info
        if lay.covar_module == 'NN':
            lo, _ = lay.block_range('kernel_nn.')
            self._ws['k'] = L.mlp_bwd(batch.x, P, theta[:, lo:], D, P, lay.input_dim, list(lay.kernel_nn_layers),
                                      lay.feature_dim, d_z, grad[:, lo:], D, False, B, n, self._ws.get('k'))
        if lay.mean_module == 'NN':
            lo, _ = lay.block_range('mean_nn.')
            self._ws['m'] = L.mlp_bwd(batch.x, P, theta[:, lo:], D, P, lay.input_dim, list(lay.mean_nn_layers), 1,
                                      d_mean.reshape(B, n, 1), grad[:, lo:], D, False, B, n, self._ws.get('m'))
        # hyper-parameters (+ constant mean): sum over tasks and softplus chain rule in one launch
        L.hyper_bwd(theta, T, off_ls, f, off_os, off_noise, off_c, d_ls, d_os, d_noise, d_const, grad, kernel=lay.kernel_code, **hyper)
        return lml.reshape(T, P), grad, info

    def predict(self, theta, ctx_x, ctx_y, tst_x, want_cov=False):
        """exact posterior predictive of ONE task for every particle: mu[P,m], var[P,m], cov[P,m,m]|None
        (normalised space, observation noise included)."""
        return self.predict_tasks(theta, ctx_x.unsqueeze(0), ctx_y.reshape(1, -1), tst_x.unsqueeze(0), want_cov=want_cov)

    def predict_tasks(self, theta, ctx_x, ctx_y, tst_x, want_cov=False, theta_per_task=False):
        """the same for T tasks of equal shape in one pass: ctx_x[T,n,d], ctx_y[T,n], tst_x[T,m,d] ->
        mu[T*P,m], var[T*P,m], cov[T*P,m,m]|None, info[T*P]; problem b = t*P + p.  theta_per_task: theta is [T*P, D], rows
        t*P .. t*P+P-1 belong to task t (fresh posterior samples per task)"""
        rows = theta.shape[0]
        T, n = ctx_x.shape[0], ctx_x.shape[1]
        m = tst_x.shape[1]
        P = rows // T if theta_per_task else rows
        ls, os_, noise = self._hypers(theta)
        zc, zc_div, mc, mode = self._features(theta, ctx_x.contiguous(), T, n, theta_per_task)
        zt, zt_div, mt, _ = self._features(theta, tst_x.contiguous(), T, m, theta_per_task)
        return L.gp_predict(zc, zc_div, mc, mode, ctx_y.contiguous(), P, zt, zt_div, mt, ls, os_, noise, T * P, rows, want_cov=want_cov,
                            kernel=self.layout.kernel_code)

    def loo_tasks(self, theta, ctx_x, ctx_y, n_valid=None, theta_per_task=False):
        """leave-one-out predictive of T tasks of equal shape for every parameter row, without a refit: ctx_x[T,n,d], ctx_y[T,n],
        n_valid int32 [T] | None -> mu[T*P,n], var[T*P,n] (the GP conditioned on the task's other points, evaluated at point i;
        normalised space, observation noise included), lpd[T*P] (mean LOO log-density over the task's points), info[T*P];
        problem b = t*P + p.  theta_per_task as predict_tasks.  One fused launch (L.gp_loo); n <= L.gp_loo_max_n(dtype)."""
        rows = theta.shape[0]
        T, n = ctx_x.shape[0], ctx_x.shape[1]
        P = rows // T if theta_per_task else rows
        ls, os_, noise = self._hypers(theta)
        z, z_div, mean, mode = self._features(theta, ctx_x.contiguous(), T, n, theta_per_task)
        return L.gp_loo(z, z_div, mean, mode, ctx_y.contiguous(), P, ls, os_, noise, T * P, rows, n_valid=n_valid,
                        kernel=self.layout.kernel_code)

    # -- conditioned posterior: condition once, predict many times, append points (csrc/gp_cond.hip) --------------------------------
    def condition(self, theta, ctx_x, ctx_y, capacity=None):
        """condition ONE task's GP on ctx_x[n,d], ctx_y[n] for every parameter row of theta (B = P problems) and keep the factor:
        -> CondState with a clone of the rows, their transformed hyper-parameters (computed once), the state buffers of
        L.gp_condition with room for `capacity` points (None: L.gp_cond_max_n) and the normalised context on the device (for a
        refit).  state.info[p] < 0: that row's kernel matrix was not positive definite on any jitter rung."""
        theta = theta.detach().clone().contiguous()
        n, d = ctx_x.shape
        dt, dev = theta.dtype, theta.device
        cap = L.gp_cond_max_n(dt) if capacity is None else int(capacity)
        L._cond_limits(n, cap, dt)
        st = CondState()
        st.theta, st.hypers, st.n, st.cap = theta, self._hypers(theta), 0, cap
        st.ctx_x = torch.zeros(cap, d, dtype=dt, device=dev)
        st.ctx_y = torch.zeros(cap, dtype=dt, device=dev)
        st.ctx_x[:n], st.ctx_y[:n] = ctx_x, ctx_y.reshape(-1)
        st.bufs = self._cond_fit(st, n, None)
        st.n = n
        return st

    def _cond_fit(self, st, n, bufs):
        """L.gp_condition of the first n stored context points into bufs (None: fresh zero-filled buffers of the state's capacity)"""
        P = st.theta.shape[0]
        ls, os_, noise = st.hypers
        z, z_div, mean, mode = self._features(st.theta, st.ctx_x[:n].unsqueeze(0).contiguous(), 1, n)
        return L.gp_condition(z, z_div, mean, mode, st.ctx_y[:n].reshape(1, n).contiguous(), P, ls, os_, noise, P, P,
                              capacity=st.cap, state=bufs, kernel=self.layout.kernel_code)

    def cond_predict(self, st, tst_x, want_var=True):
        """posterior predictive of the conditioned task at tst_x[m,d] for every parameter row: mu[P,m], var[P,m] (normalised space,
        observation noise included) -- no factorisation, one launch over P x ceil(m / 64) workgroups"""
        P = st.theta.shape[0]
        m = tst_x.shape[0]
        ls, os_, noise = st.hypers
        zt, zt_div, mt, mode = self._features(st.theta, tst_x.unsqueeze(0).contiguous(), 1, m)
        return L.gp_cond_predict(st.bufs, st.n, zt, zt_div, mt, mode, ls, os_, noise, P, P, want_var=want_var,
                                 kernel=self.layout.kernel_code)

    def cond_append(self, st, x_new, y_new):
        """append x_new[k,d], y_new[k] to the conditioned task in place (O(n^2) per point and row) -> fail int32 [P] on the device;
        rows whose update was refused need cond_refit.  Raises before anything changes when the capacity is exceeded."""
        P = st.theta.shape[0]
        k = x_new.shape[0]
        if k < 1 or st.n + k > st.cap:
            raise RuntimeError('appending %d point(s) to %d exceeds the capacity of %d of this conditioned GP (limit of %d points for %s)'
                               % (k, st.n, st.cap, L.gp_cond_max_n(st.theta.dtype), st.theta.dtype))
        ls, os_, noise = st.hypers
        z, z_div, mean, mode = self._features(st.theta, x_new.unsqueeze(0).contiguous(), 1, k)
        fail = L.gp_cond_append(st.bufs, st.n, z, z_div, mean, mode, y_new.reshape(1, k).contiguous(), P, ls, os_, noise, P, P,
                                kernel=self.layout.kernel_code)
        st.ctx_x[st.n:st.n + k], st.ctx_y[st.n:st.n + k] = x_new, y_new.reshape(-1)
        st.n += k
        return fail

    def cond_refit(self, st):
        """condition again on all st.n stored points, from scratch (the jitter ladder applies), into FRESH buffers that replace the
        state's only when the launch has been issued: the state is never half-updated"""
        st.bufs = self._cond_fit(st, st.n, None)
        return st

    # -- pathwise posterior function draws on the conditioned state (csrc/gp_path.hip) -----------------------------------------------
    def cond_paths(self, st, base):
        """fit S posterior function draws per parameter row to the conditioned task: base = (omega [D,f], phase [D], w [P,S,D],
        eps [P,S,n]) on the device (paths.draw_base) -> PathSnap, a snapshot that shares nothing with st: its own copy of the rows,
        the hyper-parameters, zs[:, :n], info, the base, and v [P,S,n] of L.gp_path_fit (one launch, no factorisation)"""
        P, n = st.theta.shape[0], st.n
        omega, phase, w, eps = base
        ls, os_, noise = st.hypers
        snap = PathSnap()
        snap.v = L.gp_path_fit(st.bufs, n, omega, phase, w, eps, os_, noise, P, P, kernel=self.layout.kernel_code)
        snap.theta, snap.n = st.theta.clone(), n
        snap.hypers = tuple(None if h is None else h.clone() for h in st.hypers)
        snap.zs, snap.info = st.bufs[0][:, :n].contiguous(), st.bufs[4].clone()
        snap.omega, snap.phase, snap.w, snap.eps = (t.clone() for t in base)
        return snap

    def cond_paths_eval(self, snap, tst_x):
        """the draws of a PathSnap at tst_x[m,d] -> [P,S,m] in normalised space (the latent function: no observation noise); the test
        features and means as cond_predict takes them, one launch over P x ceil(m / 64) x ceil(S / 64) workgroups"""
        P = snap.theta.shape[0]
        m = tst_x.shape[0]
        ls, os_, _ = snap.hypers
        zt, zt_div, mt, mode = self._features(snap.theta, tst_x.unsqueeze(0).contiguous(), 1, m)
        return L.gp_path_eval(snap.zs, snap.n, snap.v, snap.omega, snap.phase, snap.w, snap.info, zt, zt_div, mt, mode, ls, os_, P, P,
                              kernel=self.layout.kernel_code)

    def cond_paths_argmax(self, snap, tst_x, largest=True, mask=None, chunk=None):
        """per draw of a PathSnap, the eligible point of tst_x[m,d] at which cond_paths_eval's value is greatest (largest) or smallest
        -> (val [P,S] in normalised space, idx int64 [P,S]; -1 / NaN where nothing is eligible), by the rule of L.gp_path_argmax.
        mask: bool [m] on the device, True = eligible.  The pool is streamed in chunks of `chunk` candidates (None:
        PATH_ARGMAX_CHUNK): per chunk the test features of that chunk only and one L.gp_path_argmax that merges into the running
        pair, so neither [P,m,f] nor [P,S,m] exists for m > chunk"""
        from .paths import chunk_ranges
        P = snap.theta.shape[0]
        m = tst_x.shape[0]
        ls, os_, _ = snap.hypers
        best = None
        for lo, hi in chunk_ranges(m, PATH_ARGMAX_CHUNK if chunk is None else chunk):
            zt, zt_div, mt, mode = self._features(snap.theta, tst_x[lo:hi].unsqueeze(0).contiguous(), 1, hi - lo)
            best = L.gp_path_argmax(snap.zs, snap.n, snap.v, snap.omega, snap.phase, snap.w, snap.info, zt, zt_div, mt, mode, ls, os_,
                                    P, P, kernel=self.layout.kernel_code, largest=largest,
                                    mask=None if mask is None else mask[lo:hi], idx_base=lo, first=lo == 0, best=best)
        return best

    # -- analytic acquisition on the conditioned predictive (csrc/acq.hip) -----------------------------------------------------------
    def cond_acq(self, st, tst_x, kind, best_n=0.0, xi_n=0.0, beta=2.0, sign=1, latent=True, mask=None, chunk=None, want_values=False):
        """score tst_x[m,d] with the acquisition `kind` of the equal-weight mixture of the conditioned task's parameter rows and find
        its best eligible point -> (val [1] in normalised space, idx int64 [1]; -1 / NaN where nothing is eligible, values [m] | None),
        by the rule of L.mixture_acq.  latent: the rows' noise is taken off their predictive variance (the latent function).
        mask: bool [m] on the device, True = eligible.  The pool is streamed in chunks of `chunk` candidates (None: PATH_ARGMAX_CHUNK):
        per chunk one cond_predict of that chunk and one L.mixture_acq that merges into the running pair, so at most [P, chunk]
        moments are ever resident.  'mean' / 'ucb' with sign = -1 look for the smallest value, everything else for the greatest."""
        from .paths import chunk_ranges
        P = st.theta.shape[0]
        m = tst_x.shape[0]
        noise = st.hypers[2].reshape(-1).contiguous() if latent else None
        largest = not (kind in ('mean', 'ucb') and sign == -1)
        best, vals = None, []
        for lo, hi in chunk_ranges(m, PATH_ARGMAX_CHUNK if chunk is None else chunk):
            mu, var = self.cond_predict(st, tst_x[lo:hi])
            bv, bi, v = L.mixture_acq(mu, var, 1, P, kind, best_n, xi_n, beta, sign, noise=noise,
                                      mask=None if mask is None else mask[lo:hi], want_values=want_values, largest=largest,
                                      idx_base=lo, first=lo == 0, best_pair=best)
            best = (bv, bi)
            if want_values:
                vals.append(v[0])
        values = None if not want_values else (vals[0] if len(vals) == 1 else torch.cat(vals))
        return best[0], best[1], values


PATH_ARGMAX_CHUNK = 131072       # candidates per launch of cond_paths_argmax: [P, chunk, f] features is all that is ever resident


class PathSnap:
    """what GPEngine.cond_paths keeps of one set of draws: theta [P,D], hypers, zs [P,n,f], info [P], n, the base (omega, phase, w,
    eps) and the fitted v [P,S,n]"""
    __slots__ = ('theta', 'hypers', 'zs', 'info', 'n', 'omega', 'phase', 'w', 'eps', 'v')


class CondState:
    """what GPEngine.condition keeps of one task: theta [P,D] (a clone), hypers (lengthscale, outputscale, noise), bufs = (zs, resid,
    X, alpha, info) of L.gp_condition, n points in use of cap, and the normalised context ctx_x[cap,d], ctx_y[cap] for a refit"""
    __slots__ = ('theta', 'hypers', 'bufs', 'n', 'cap', 'ctx_x', 'ctx_y')

    @property
    def info(self):
        return self.bufs[4]
