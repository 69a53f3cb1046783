"""PACOH-SVGD on MI355X: API of GPRegressionMetaLearnedSVGD (meta_learn/GPR_meta_svgd.py:14-230).
One svgd_step = [MLP fwd x2] -> fused GP LML fwd+bwd over tasks x particles -> [MLP bwd x2] ->
hyper-prior grad -> SVGD phi -> Adam, all HIP kernels on one stream; with torch.distributed
initialised, tasks are sharded over ranks and the score is all-reduced once per step (RCCL)."""
import os

import numpy as np
import torch

from . import _lib as L
from . import parallel
from .abstract import RegressionModelMetaLearned
from .engine import AsyncUploader, GPEngine, ParamLayout, StepDriver, StepMode, TaskBatch
from .util import StepLR


def consume_vectorized_gp_init_rng(layout):
    """Advance the torch CPU generator exactly as building the reference's VectorizedGP does (every
    LinearVectorized draws normal(in*out), weight.uniform_, bias.uniform_; models.py:283-293; mean_nn
    before kernel_nn, random_gp.py:33-46) so that seeded runs draw the same initial particles."""
    def net(in_dim, out_dim, layers):
        prev = in_dim
        for size in list(layers) + [out_dim]:
            w = torch.normal(0, 1, size=(prev * size,))
            w.uniform_(-1.0, 1.0)
            torch.empty(size).uniform_(-1.0, 1.0)
            prev = size
    if layout.mean_module == 'NN':
        net(layout.input_dim, 1, layout.mean_nn_layers)
    if layout.covar_module == 'NN':
        net(layout.input_dim, layout.feature_dim, layout.kernel_nn_layers)


def sample_hyper_prior(layout, prior_mean, prior_std, n):
    """CatDist.sample: block after block torch.normal(loc.expand, scale.expand) (models.py:183-184)"""
    blocks = []
    for name, (lo, hi) in layout.slices.items():
        loc = prior_mean[lo:hi].expand(n, hi - lo)
        scale = prior_std[lo:hi].expand(n, hi - lo)
        blocks.append(torch.normal(loc, scale))
    return torch.cat(blocks, dim=-1)


def harmonic_pre_factor(sizes):
    """m~/(m~+T), m~ = harmonic mean of the batch's dataset sizes, T = batch length (random_gp.py:209-212)"""
    sizes = np.asarray(sizes, dtype=np.float32)
    hm = np.float32(1.0) / np.mean(np.float32(1.0) / sizes, dtype=np.float32)
    return float(hm / (hm + np.float32(len(sizes))))


class _RandomGPLearner(StepDriver, RegressionModelMetaLearned):
    """what SVGD and VI share: RandomGPMeta semantics (random_gp.py:116-222) on the device engine"""

    def _setup_random_gp(self, meta_train_data, mean_module, covar_module, mean_nn_layers, kernel_nn_layers,
                         task_batch_size):
        assert mean_module in ['NN', 'constant'] and covar_module in ['NN', 'SE']
        meta_train_data = list(meta_train_data)
        if task_batch_size < 1:
            self.task_batch_size = len(meta_train_data)
        else:
            self.task_batch_size = min(task_batch_size, len(meta_train_data))
        self._check_meta_data_shapes(meta_train_data)
        self._compute_normalization_stats(meta_train_data)
        # NB: the reference never forwards feature_dim to VectorizedGP -> always 2 (GPR_meta_svgd.py:167-170)
        self.layout = ParamLayout(self.input_dim, mean_module, covar_module, mean_nn_layers, kernel_nn_layers,
                                  feature_dim=2, with_outputscale=False)
        self.engine = GPEngine(self.layout, noise_floor=0.0)         # plain softplus (random_gp.py:73)
        pm, ps = self.layout.hyper_prior_mean_std(self.weight_prior_std, self.bias_prior_std)
        self._prior_mean_cpu, self._prior_std_cpu = pm, ps
        self.prior_mean = pm.to(self.dtype).to(self.device)
        self.prior_std = ps.to(self.dtype).to(self.device)
        consume_vectorized_gp_init_rng(self.layout)
        return meta_train_data

    def _setup_tasks(self, meta_train_data):
        tasks = [self._prepare_data_per_task(x, y) for x, y in meta_train_data]
        self.tasks = TaskBatch(tasks, self.device, self.dtype)

    def _sample_task_batch(self):
        """global with-replacement draw from the shared seed (GPR_meta_svgd.py:102), then this rank's shard"""
        idx = self._take_idx(1)[0]
        pre = harmonic_pre_factor(self.tasks.sizes[idx])
        local = parallel.shard(idx)
        return local, pre

    # ---- the training loop's steps, captured in hipGraphs ---------------------------------------------------------------------
    # One step is ~12 launches; issued one by one from Python that is ~0.35 ms of host time, more than the GPU needs for a small
    # configuration or a 1/8 shard of a large one.  The step's kernels read everything that changes between steps (task draws,
    # pre-factor, learning rate, Adam's bias corrections) from device buffers filled for up to GRAPH_CHUNK steps at once
    # (engine.StepFeed), so the launch sequence is captured once and replayed.  With several ranks the step is two graphs around
    # the eager all-reduce of the packed score buffer.  PACOH_NO_GRAPH=1 runs the very same launch sequence eagerly.
    def _step_scalars(self, idx):
        """the steps' scalar rows of the task draws idx [k, B]"""
        k = idx.shape[0]
        # harmonic pre-factor per step (random_gp.py:209-212); tasks of one size: every row is the same computation on the same
        # numbers -- done once
        rows = idx if self.tasks.ragged else idx[:1]
        sizes = self.tasks.sizes[rows].astype(np.float32)
        hm = np.float32(1.0) / np.mean(np.float32(1.0) / sizes, axis=1, dtype=np.float32)
        pre = (hm / (hm + np.float32(self.task_batch_size))).astype(np.float64)
        if not self.tasks.ragged:
            pre = np.repeat(pre, k)
        return L.step_scalar_rows(pre, self.lr_scheduler.lrs(k), self.opt_step + 1)

    # Under-filled grids (round 6): the reference's own launchers run 2 tasks x 10 particles / samples of 20 points per step -- 20 GP
    # problems, for which networks forward -> GP -> networks backward -> slab reduction are four kernel latencies.  There the
    # likelihood half of a step is pacoh_svgd_task_step: one workgroup per (task, parameter row) does all three stages with the
    # activations in LDS, then the slab reduction -- two launches.  It wins while all its workgroups are resident at once (one round of
    # ~20 us latency chains: up to 256-768 problems by network size, profiles/r06_task_fused_crossover.txt); the library's workspace
    # query answers that question for the device at hand, larger grids stay on the throughput kernels.

    def _setup_task_fused(self, rows, tb_local):
        """-> workspace of L.svgd_task_step for `rows` parameter rows x tb_local tasks per step, or None (general launch sequence):
        fp32, RBF GP kernel, a shape inside the task-fused kernel's plan whose workgroups are all resident at once.
        PACOH_SVGD_TASK_FUSED=0 / 1: never / wherever the plan allows (tests, A/B)"""
        self._task_plan = self._task_ws = None
        force = os.environ.get('PACOH_SVGD_TASK_FUSED')
        if force == '0' or tb_local < 1 or self.dtype != torch.float32 or L.FORCE_DENSE:
            return None
        plan = L.MapPersistPlan(self.layout, self.tasks, tb_local, 0.0, [(0, self.layout.D)], self.dtype)
        ws = L.svgd_task_workspace(plan, rows, tb_local, self.device, any_size=force == '1')
        if ws is not None:
            self._task_plan, self._task_ws = plan, ws
        return ws

    # Duplicate draws (the tasks of a step are drawn WITH replacement: _take_idx).  A draw of 1024 from 1024 tasks holds ~647 distinct
    # ones; the networks, the GP and their backward of a repeated draw recompute the same numbers on the same inputs.  The feed then
    # hands the kernels each draw's distinct tasks with their multiplicities (engine.distinct_rows; include/pacoh_gp.h,
    # pacoh_active_tasks): sum_{draws t} g(t, p) = sum_{distinct u} count_u g(u, p).  The pre-factor keeps using the draw itself.
    DEDUP_MIN_PROBLEMS = 4096    # one resident round of the GP kernel (4 waves x 4 SIMDs x 256 CUs): below it the three large kernels
                                 # are a single round of workgroups, and fewer problems do not shorten a launch

    def _setup_dedup(self, rows, tb_local):
        """switch the step feed to distinct tasks where the step runs on the kernels that take them -- fp32, both networks on the
        fused kernels, the GP on the register-resident kernel (RBF features, n <= 128, f <= 4), not the task-fused small-grid step --
        and has at least DEDUP_MIN_PROBLEMS (task, parameter row) problems.  PACOH_SVGD_DEDUP=0 / 1: never / wherever eligible
        (tests, A/B).  The same for every launch sequence of the step (pipelined or not, replayed or eager)."""
        force = os.environ.get('PACOH_SVGD_DEDUP')
        lay = self.layout
        if force == '0' or tb_local < 1 or self.dtype != torch.float32 or self._task_ws is not None or L.FORCE_DENSE:
            return
        if self.engine._paired_nets() is None or lay.kernel_code != L.KERNEL_RBF or self.tasks.n > 128 or lay.feature_dim > 4:
            return
        if not all(L.mlp_fused_path(tb_local * rows, rows, self.tasks.n, lay.input_dim, list(lay.mean_nn_layers), d_out, self.dtype)
                   for d_out in (1, lay.feature_dim)):
            return
        if force == '1' or tb_local * rows >= self.DEDUP_MIN_PROBLEMS:
            self._feed.enable_dedup(self.tasks.T)

    def _idx_uploader(self):
        up = getattr(self, '_idx_up', None)
        if up is None:
            up = self._idx_up = AsyncUploader(self.device, torch.int64)
        return up

    def _log_prob_and_score(self, theta, idx_local, pre_factor, with_prior=True):
        """RandomGPMeta.log_prob and its gradient (random_gp.py:204-222; svgd.py:15-16):
        log_prob[p] = prior_factor*log p(theta_p) + pre_factor * sum_t mll[t,p]
        (with_prior=False: the likelihood term and its score only -- the fused SVGD update adds the prior's score itself)"""
        P, D = theta.shape
        packed, score, lik = parallel.packed_score_buffer(P, D, theta.dtype, theta.device)   # lik = pre_factor * sum_t mll[t,p]
        if len(idx_local) > 0:
            batch = self.tasks.select(self._idx_uploader().upload(idx_local))
            self.engine.lml_and_grad(theta, batch, weight=pre_factor, lik_out=lik, lik_scale=pre_factor, grad_out=score)
        else:
            packed.zero_()
        lik, score = parallel.all_reduce_sum_(lik, score, packed)     # ONE exchange per step, no packing copies
        if not with_prior:
            return lik, score
        logprior = L.prior_logprob_grad(theta, self.prior_mean, self.prior_std, score, self.prior_factor)
        L.axpy(lik, logprior, self.prior_factor)                      # lik += prior_factor * log p(theta)
        return lik, score


class GPRegressionMetaLearnedSVGD(_RandomGPLearner):

    def __init__(self, meta_train_data, num_iter_fit=10000, feature_dim=1,
                 prior_factor=0.01, weight_prior_std=0.5, bias_prior_std=3.0,
                 covar_module='NN', mean_module='NN', mean_nn_layers=(32, 32), kernel_nn_layers=(32, 32),
                 optimizer='Adam', lr=1e-3, lr_decay=1.0, kernel='RBF', bandwidth=None, num_particles=10,
                 task_batch_size=-1, normalize_data=True, random_seed=None):
        """Arguments as in the reference (GPR_meta_svgd.py:16-44)."""
        super().__init__(normalize_data, random_seed)
        assert mean_module in ['NN', 'constant', 'zero'] and covar_module in ['NN', 'SE']
        assert optimizer in ['Adam', 'SGD']
        if kernel not in ('RBF', 'IMQ'):                       # GPR_meta_svgd.py:173-179
            raise NotImplementedError
        self.kernel = kernel
        assert num_particles <= L.SVGD_MAX_PARTICLES, 'too many particles for the SVGD kernels'
        self.num_iter_fit, self.prior_factor, self.feature_dim = num_iter_fit, prior_factor, feature_dim
        self.weight_prior_std, self.bias_prior_std = weight_prior_std, bias_prior_std
        self.num_particles, self.bandwidth, self.optimizer_name = num_particles, bandwidth, optimizer
        meta_train_data = self._setup_random_gp(meta_train_data, mean_module, covar_module, mean_nn_layers,
                                                kernel_nn_layers, task_batch_size)
        # initial particles = one draw from the hyper-prior (GPR_meta_svgd.py:182)
        particles = sample_hyper_prior(self.layout, self._prior_mean_cpu, self._prior_std_cpu, num_particles)
        self.particles = particles.to(self.dtype).to(self.device).contiguous()
        self.exp_avg = torch.zeros_like(self.particles)
        self.exp_avg_sq = torch.zeros_like(self.particles)
        self.opt_step = 0
        self.lr_scheduler = StepLR(lr, 1000, lr_decay)
        self._svgd_ws = None
        self._step_mode = StepMode()
        self._setup_tasks(meta_train_data)
        self.fitted = False

    # ---- one SVGD step = likelihood body -> [all-reduce] -> update body ----------------------------------------------------------
    _STEP_STATE = ('particles', 'exp_avg', 'exp_avg_sq')

    def _setup_step(self, tb_local):
        if self._feed is not None and self._feed.tb == tb_local:
            return
        P, D = self.particles.shape
        self._score, self._lik = self._new_step(tb_local, P, self.GRAPH_CHUNK)      # score [P, D] | lik [P]
        self._bw_out = torch.zeros(1, dtype=self.dtype, device=self.device)
        self._svgd_ws = L.svgd_update_workspace(self.particles, self._svgd_ws)
        # Five launches per step instead of six (csrc/step_tail.h): the distance matrix rides in the forward launch, the next step's
        # scalars and task batch are fetched by the update launch.  A rank without tasks of its own has no forward launch: it keeps
        # the step_begin launch.  PACOH_SVGD_PIPELINE=0: the round-2 launch sequence (A/B measurements, bit-identity tests)
        # (the IMQ particle kernel has its own launch sequence: _body_update_imq)
        self._pipelined = tb_local > 0 and self.kernel == 'RBF' and os.environ.get('PACOH_SVGD_PIPELINE', '1') != '0'
        if self.kernel == 'IMQ':
            self._imq_phi = torch.empty_like(self.particles)
            self._imq_h = torch.empty(D, dtype=self.dtype, device=self.device) if self.bandwidth is None else None
            self._imq_ws = L.svgd_imq_workspace(self.particles)
        self._setup_task_fused(P, tb_local)
        self._setup_dedup(P, tb_local)
        if self._pipelined:
            self._feed.pipeline(self.tasks, self.engine, self.particles)
        # median bandwidth computed beside the hyper-parameter reduction instead of inside the update (P <= 64: one wavefront's sort)
        self._bw_ahead = self._pipelined and self.bandwidth is None and P <= 64

    def _body_likelihood(self):
        """score[P,D] = d/d theta_p sum_t mll[t,p] over this rank's tasks (unscaled), lik[P] the sums themselves"""
        if self._pipelined and self._task_ws is not None:
            L.svgd_task_step(self._task_plan, self.particles, self._feed.batch, self._feed.hyp, self._score, self._lik, 1.0, self._fail,
                             self._task_ws, svgd=(self.particles, self._svgd_ws, self._feed.ctr, self._bw_ahead))
            return
        if self._pipelined:
            self.engine.lml_and_grad(self.particles, self._feed.batch, weight=1.0, lik_out=self._lik, lik_scale=1.0,
                                     grad_out=self._score, fail_flag=self._fail, hypers=self._feed.hyp,
                                     svgd_tail=(self.particles, self._svgd_ws, self._feed.ctr, self._bw_ahead),
                                     active=self._feed.active())
            return
        # select + gather + hyper transforms + the particles' distance matrix: one launch; the counter is advanced by the update
        # (IMQ: no distance matrix -- its bandwidths are per-dimension medians; the counter is advanced by the Adam launch, or
        # behind this one for SGD)
        if self.kernel == 'IMQ':
            batch, hyp = self._feed.begin(self.tasks, self.engine, self.particles, advance=self.optimizer_name != 'Adam')
        else:
            batch, hyp = self._feed.begin(self.tasks, self.engine, self.particles, advance=False, svgd=(self.particles, self._svgd_ws))
        if batch is None:
            self._packed.zero_()
            return
        if self._task_ws is not None:
            L.svgd_task_step(self._task_plan, self.particles, batch, hyp, self._score, self._lik, 1.0, self._fail, self._task_ws)
            return
        self.engine.lml_and_grad(self.particles, batch, weight=1.0, lik_out=self._lik, lik_scale=1.0, grad_out=self._score,
                                 fail_flag=self._fail, hypers=hyp, active=self._feed.active())

    def _body_update(self):
        """prior score + pre-factor + bandwidth + phi + optimizer in one launch (distances: _body_likelihood), particles updated
        in place, step counter advanced"""
        if self.kernel == 'IMQ':
            return self._body_update_imq()
        self.last_bandwidth = self._bw_out
        if self._pipelined:
            L.svgd_update_next(self.particles, self._score, self.prior_mean, self.prior_std, self.prior_factor, self.bandwidth,
                               self.optimizer_name, self.exp_avg, self.exp_avg_sq, self._svgd_ws, self._bw_out, self._feed, self.tasks,
                               self._feed.hyper, bandwidth_ready=self._bw_ahead)
            return
        _, self._svgd_ws = L.svgd_update_dev(self.particles, self._score, self.prior_mean, self.prior_std, self.prior_factor,
                                             self.bandwidth, self.optimizer_name, self._feed.sc, self.exp_avg, self.exp_avg_sq,
                                             workspace=self._svgd_ws, bw_out=self._bw_out, dist_done=True,
                                             step_counter=self._feed.ctr)
        self.last_bandwidth = self._bw_out

    def _body_update_imq(self):
        """SVGD.step with the IMQ particle kernel (svgd.py:12-28, 58-77) on the step feed: every step-dependent scalar (pre-factor,
        learning rate, Adam's bias corrections) is read from the feed's selected row in device memory, so that the launch
        sequence is captured and replayed like the RBF one.  score <- pre * score + prior_factor * d log prior (random_gp.py:
        204-222), -phi from pacoh_svgd_phi_imq (per-dimension median bandwidths incl. the gradient through them), optimizer step."""
        sc = self._feed.sc
        L.prior_score_dev(self.particles, self.prior_mean, self.prior_std, self._score, self.prior_factor,
                          sc[L.SC_SCORE_SCALE:L.SC_SCORE_SCALE + 1])
        neg_phi, self.last_bandwidth, self._imq_ws = L.svgd_phi_imq(self.particles, self._score, bandwidth=self.bandwidth, neg=True,
                                                                    workspace=self._imq_ws, phi_out=self._imq_phi, h_out=self._imq_h)
        if self.optimizer_name == 'Adam':
            L.adam_step_dev(self.particles, neg_phi, self.exp_avg, self.exp_avg_sq, sc[L.SC_ADAM:L.SC_ADAM + 4],
                            step_counter=self._feed.ctr)
        else:
            L.scale_dev(neg_phi, sc[L.SC_LR:L.SC_LR + 1])          # particles -= lr * (-phi)
            L.axpy(self.particles, neg_phi, -1.0)

    def svgd_step(self, idx_local, pre_factor):
        """SVGD.step (meta_learn/svgd.py:25-28) on an explicit task draw: particles.grad = -phi; optimizer.step()"""
        self._setup_step(len(idx_local))
        self.opt_step += 1
        self._feed.upload(np.asarray(idx_local).reshape(1, -1) if len(idx_local) > 0 else None,
                          [L.step_scalars(pre_factor, self.lr_scheduler.lr, self.opt_step)])
        self._prologue()
        self._run_step(False)

    def meta_fit(self, valid_tuples=None, verbose=True, log_period=500, n_iter=None):
        """GPR_meta_svgd.py:82-121"""
        assert (valid_tuples is None) or (all([len(valid_tuple) == 4 for valid_tuple in valid_tuples]))
        self._fit_loop(n_iter, log_period, valid_tuples, verbose, self._train_steps)
        self._check_numerics()
        self.fitted = True

    def predict(self, context_x, context_y, test_x, return_density=False):
        """GPR_meta_svgd.py:123-159: equal-weighted mixture over the particles' GP posteriors"""
        return self._predictive(self.particles, context_x, context_y, test_x, return_density)

    def _eval_params(self, **kwargs):
        return (self.particles, True, False) if not kwargs else None

    def state_dict(self):
        return {'particles': self.particles.cpu().clone(), 'exp_avg': self.exp_avg.cpu().clone(),
                'exp_avg_sq': self.exp_avg_sq.cpu().clone(), 'step': self.opt_step, 'epoch': self.lr_scheduler.epoch}

    def load_state_dict(self, state_dict):
        self.particles.copy_(state_dict['particles']); self.exp_avg.copy_(state_dict['exp_avg']); self.exp_avg_sq.copy_(state_dict['exp_avg_sq'])
        self.opt_step, self.lr_scheduler.epoch = int(state_dict['step']), int(state_dict['epoch'])
