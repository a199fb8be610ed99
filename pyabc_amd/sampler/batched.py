"""BatchedGPUSampler: one ABC-SMC generation as a few large kernel launches.

Reference loop: pyabc/sampler/singlecore.py:20-38 and
multicore_evaluation_parallel.py:14-150 call the per-candidate closure
(smc.py:588-724) until n particles are accepted, keep the first n by
evaluation id and count every evaluation.  Here a round of B candidates per
rank runs as

  propose (abc_propose / abc_local_propose, prior re-draw loop inside)
  -> simulate (VectorizedModel, e.g. abc_simulate_linear_gaussian)
  -> distance (abc_pnorm) -> accept + order-preserving compaction
     (abc_accept_compact)

with one host read of the accept count per round.  Once n are accepted the
importance weights prior / transition (smc.py:768-811) are computed for the
accepted rows only -- the N_acc x N_pop transition density on MFMA
(abc_mvn_logpdf) -- and the accepted rows are gathered across ranks.

Semantics vs. the reference: the accepted set is the first n accepted in
global candidate-index order (deterministic for any rank count), and
``nr_evaluations_`` = global index of the n-th accepted + 1, i.e. no
overshoot is counted (the reference's MulticoreEval counts its overshoot,
multicore_evaluation_parallel.py:138).  Recorded sum stats (record_rejected)
are all candidates up to that cutoff, in index order (SingleCore semantics).
"""
import logging
import math

import numpy as np

from .. import gpu
from .._native import PRIOR_KINDS
from ..distance.distance import SumStatMatrix
from ..population import ColumnarParticles, Particle, Population
from ..parameters import Parameter
from ..random_variables import host_prior_draw, host_prior_logpdf
from . import distributed as dd
from .base import Sampler

logger = logging.getLogger("Sampler")


class ColumnarSample:
    """Sample of the batched sampler (device columns, see Sample)."""

    def __init__(self, columns, recorded, recorded_keys, record_rejected, ok,
                 accepted_flags=None, records=None):
        self._cols = columns
        self._records = records              # (theta, dens, key, anc) or None
        self._recorded = recorded            # [R, S] device or None
        self._recorded_keys = recorded_keys
        self._accepted_flags = accepted_flags
        self.record_rejected = record_rejected
        self.ok = ok

    @property
    def n_accepted(self):
        return 0 if self._cols is None else len(self._cols)

    def get_accepted_population(self):
        return Population.from_columns(self._cols)

    def first_m_sum_stats(self, m):
        rec = self._recorded
        if rec is None:
            return []
        if m is not None and np.isfinite(m) and m < rec.shape[0]:
            rec = rec[: int(m)].contiguous()
        return SumStatMatrix(rec, self._recorded_keys)

    def device_records(self, m=None):
        """(theta [R, d], density [R], acceptance key [R], ancestor [R] or
        None) of the first m recorded candidates (all evaluated candidates
        up to the cutoff, accepted and rejected, in index order); None if
        the generation did not record them (StochasticAcceptor runs with
        record_rejected only)."""
        if self._records is None:
            return None
        th, dn, key, anc = self._records
        if m is not None and np.isfinite(m) and m < th.shape[0]:
            m = int(m)
            th, dn, key = th[:m], dn[:m], key[:m]
            anc = None if anc is None else anc[:m]
        return th, dn, key, anc

    @property
    def all_sum_stats(self):
        return self.first_m_sum_stats(np.inf)

    def first_m_particles(self, m):
        c = self._cols
        th = c.theta.cpu().numpy()
        w = c.weights.cpu().numpy()
        d = c.distances.cpu().numpy()
        ss = c.sum_stats.cpu().numpy()
        parts = [Particle(m=c.m, parameter=Parameter(dict(zip(c.param_names, th[i]))),
                          weight=float(w[i]),
                          accepted_sum_stats=[dict(zip(c.sum_stat_keys, ss[i]))],
                          accepted_distances=[float(d[i])])
                 for i in range(len(c))]
        m = len(parts) if m is None or not np.isfinite(m) else int(m)
        return parts[:m]


class ModelsSample(ColumnarSample):
    """ColumnarSample over several models: {m: ColumnarParticles}."""

    def __init__(self, model_columns, recorded, recorded_keys, record_rejected, ok):
        super().__init__(None, recorded, recorded_keys, record_rejected, ok)
        self._mcols = model_columns

    @property
    def n_accepted(self):
        return sum(len(c) for c in self._mcols.values())

    def get_accepted_population(self):
        return Population.from_model_columns(self._mcols)

    def first_m_particles(self, m):
        parts = self.get_accepted_population().get_list()
        return parts if m is None or not np.isfinite(m) else parts[:int(m)]


class _PinnedReader:
    """Device int64 values read on the host with one wait: queue() copies
    them into a cached pinned buffer (async copies, no concatenation kernel,
    no allocation) and records an event; wait() returns them.  Work queued
    after the event (the kept rows' regeneration) runs while the host waits."""

    def __init__(self):
        self._host = self._event = self._direct = None

    def queue(self, *pieces):
        torch = gpu.torch
        self._direct = None
        if not pieces[0].is_cuda:                  # host tensors (test doubles)
            self._direct = np.concatenate([t.reshape(-1).numpy() for t in pieces])
            return
        sizes = [t.numel() for t in pieces]
        host = self._host
        if host is None or host.numel() != sum(sizes):
            host = self._host = torch.empty(sum(sizes), dtype=torch.int64,
                                            pin_memory=True)
            self._event = torch.cuda.Event()
        off = 0
        for t, k in zip(pieces, sizes):
            host[off:off + k].copy_(t.reshape(k), non_blocking=True)
            off += k
        # the stream named by the tensor's device: record() with no stream
        # resolves the current device through torch.cuda.is_available (~40 us)
        self._event.record(torch.cuda.current_stream(pieces[0].device))

    def wait(self):
        """The queued values (numpy int64, the caller's own copy)."""
        if self._direct is not None:
            return self._direct
        self._event.synchronize()
        return self._host.numpy().copy()


class _RoundLedger:
    """Host bookkeeping of one generation's candidate rounds, the same for
    every loop that runs them: the first-n-accepted cutoff over the ranks
    (global candidate-index order), evaluations up to the n-th accepted, the
    rows each rank keeps and records per round, and the cap on recorded rows.
    Holds no device tensor but the pending cut's position."""

    def __init__(self, n, rank, ws, S, max_recorded, budget_bytes=None):
        self.n, self.rank, self.ws = n, rank, ws
        self.n_acc = self.n_eval = self.base = self.rounds = 0
        self.keeps = []         # per round: accepted rows kept by each rank
        self.rec_keeps = []     # per round: recorded rows of each rank
        self.cut = None         # ws > 1: the last round's cutoff, see finish
        # recorded rows still allowed: the first max_recorded are all that is
        # used, fewer when the device budget holds fewer rows of S statistics
        self.rec_left = max_recorded
        self.records_truncated = False
        self._budget_bytes = None           # set: the budget is the cap
        if budget_bytes is not None:
            budget_rows = budget_bytes // (8 * max(S, 1))
            if budget_rows < max_recorded:
                self._budget_bytes = budget_bytes
            self.rec_left = min(max_recorded, budget_rows)

    @property
    def need(self):
        return self.n - self.n_acc

    def settle(self, counts, B, idx, pos, recording):
        """Book one completed round of B candidates per rank.  counts: the
        accept count of every rank (host); idx: this rank's accepted
        positions (device, read only by a pending cut); pos: on one rank the
        position of the need-th accepted (meaningful when the round completes
        the sample); recording: whether the round wrote its candidates' rows.
        Returns (rows this rank keeps, rows this rank records); the latter is
        None while a multi-rank cut is pending (finish gives it)."""
        ws = self.ws
        keep = dd.cutoff(counts, self.need)
        total_keep = int(keep.sum())
        # evaluations up to the cutoff (global order); rec_all = recorded
        # rows of every rank this round (identical on all ranks)
        rec_all = np.full(ws, B if recording else 0, dtype=np.int64)
        if self.n_acc + total_keep >= self.n:
            c_rank = int(np.nonzero(keep)[0][-1])
            if ws > 1:
                # the cutoff position travels in the generation's packed
                # row gather (_assemble), not in a collective of its own
                self.cut = self._pending_cut(idx, int(keep[c_rank]), c_rank, B)
                evaluated = 0
                if recording:
                    rec_all = None
            else:
                evaluated = c_rank * B + pos + 1
                if recording:
                    rec_all = self._rows_up_to(c_rank, pos, B)
        else:
            evaluated = ws * B
        if rec_all is not None:
            rec_all = self._cap_records(rec_all)
        self.rec_keeps.append(rec_all)
        self.keeps.append(keep)
        self.n_acc += total_keep
        self.n_eval += evaluated
        self.base += ws * B
        self.rounds += 1
        return int(keep[self.rank]), (None if rec_all is None
                                      else int(rec_all[self.rank]))

    def finish(self, gathered):
        """Resolve the pending cut once the packed row gather has brought the
        cut rank's position (gathered[rank]): adds the last round's
        evaluations up to the n-th accepted (global order) and caps that
        round's recorded rows like every round's.  Returns the rows this
        rank's recorded pieces of that round are trimmed to (None: nothing
        to trim)."""
        if self.cut is None:
            return None
        c_rank, B = self.cut["c_rank"], self.cut["B"]
        pos = int(gathered[c_rank])
        self.n_eval += c_rank * B + pos + 1
        if self.rec_keeps[-1] is not None:
            return None
        rec_all = self._cap_records(self._rows_up_to(c_rank, pos, B))
        self.rec_keeps[-1] = rec_all
        return int(rec_all[self.rank])

    def _rows_up_to(self, c_rank, pos, B):
        """Recorded rows per rank of the round cut at c_rank's position pos."""
        rec_all = np.full(self.ws, B, dtype=np.int64)
        rec_all[c_rank] = pos + 1
        rec_all[c_rank + 1:] = 0
        return rec_all

    def _pending_cut(self, idx, k, c_rank, B):
        """The completing round of a multi-rank generation: the cut rank's
        local position of its last (k-th) kept candidate stays on the device
        (no host read, no collective of its own) and rides in the packed row
        gather of _assemble; every other rank sends -1."""
        if self.rank == c_rank:
            pos = idx[k - 1:k].to(gpu.F64)
        else:
            pos = gpu.torch.full((1,), -1.0, dtype=gpu.F64, device=idx.device)
        return dict(c_rank=c_rank, B=int(B), pos=pos)

    def _cap_records(self, rec_all):
        """Keep only the first rec_left recorded candidates in global order
        (round-major, then rank): the round's rows per rank after the cap."""
        if not np.isfinite(self.rec_left):
            return rec_all
        out = np.zeros_like(rec_all)
        left = int(self.rec_left)
        for q in range(len(rec_all)):
            out[q] = min(int(rec_all[q]), left)
            left -= int(out[q])
        if left == 0 and out.sum() < rec_all.sum() and self._budget_bytes is not None:
            if not self.records_truncated:
                logger.warning("recorded sum stats exceed record_device_budget_bytes "
                               "(%d); keeping the first rows only", self._budget_bytes)
            self.records_truncated = True
        self.rec_left = left
        return out


class _OneModelSource:
    """Candidate source of a one-model generation: proposals of the cached
    proposal-only CandidateRound (gpu.propose / propose_device where it has
    none), the model's own simulate_batch."""

    def __init__(self, sampler, spec, seed, gen, dev, all_accepted):
        self.sampler, self.spec, self.dev = sampler, spec, dev
        self.seed, self.gen, self.all_accepted = seed, gen, all_accepted
        self.d = len(spec.param_names)         # the round size's dimension
        # t = 0: the host-scipy leg draws its coordinates as ppf of the
        # candidates' own prior-stream uniforms
        self.host_draw = (getattr(spec, "host_prior", None)
                          if spec.transition is None else None)

    def propose(self, lo, B):
        """(the candidates' columns, att)."""
        theta, lp, anc, att = self.sampler._propose(self.spec, B, self.seed,
                                                    self.gen, lo, self.d)
        if self.host_draw:
            host_prior_draw(theta, att, self.host_draw, self.seed, self.gen, lo)
        return dict(theta=theta, lp=lp, anc=anc), att

    def simulate(self, cand, lo):
        return self.spec.model.simulate_batch(cand["theta"], self.seed, self.gen, lo)

    def kept_columns(self, cand):
        """The candidates' columns that ride with a kept row."""
        return {k: v for k, v in cand.items() if v is not None}

    def complete(self, got, att, unfiltered):
        """The prior log-density of the kept rows, where the proposal left
        it out: the bits the proposal kernel would have written (same device
        function)."""
        if "lp" in got:
            return
        spec = self.spec
        got["lp"] = gpu.prior_logpdf(got["theta"], spec.prior_kind, spec.prior_params)
        if unfiltered and att is not None:
            # rows 0..k-1 are kept unfiltered, including proposals that
            # exhausted max_attempts: their last draw's density is not the
            # proposal's, and the proposal kernel would have written -inf
            # (weight 0)
            gpu.mask_gave_up(got["lp"], att[:got["lp"].numel()],
                             self.sampler.max_attempts, -np.inf)

    def assemble(self, kept, led):
        """(population columns, the ranks' cutoff positions or None, the
        source's own last_stats keys)."""
        cols, gathered = self.sampler._assemble(self.spec, kept, self.dev, self.d,
                                                self.all_accepted, led)
        return cols, gathered, {}

    def sample(self, cols, recorded, record, ok, records):
        if recorded is None and cols is not None:
            recorded = cols.sum_stats
        return ColumnarSample(cols, recorded, self.spec.sum_stat_keys, record, ok,
                              records=records)


class _GridSource(_OneModelSource):
    """Candidate source of a one-model generation over integer parameters: a
    grid prior (abc_grid_prior_draw at t = 0, abc_grid_prior_logpmf on the
    kept rows) and DiscreteRandomWalkTransition.propose_device afterwards.
    It builds no CandidateRound and never takes the fused round; the staged
    loop, the ledger, the accept tails and the ranks' gather are
    _OneModelSource's."""

    def __init__(self, sampler, spec, seed, gen, dev, all_accepted):
        super().__init__(sampler, spec, seed, gen, dev, all_accepted)
        self.prior = spec.grid_prior

    def propose(self, lo, B):
        if self.spec.transition is None:
            theta = self.prior.draw(self.seed, self.gen, lo, B)
            return dict(theta=theta, lp=None, anc=None), None
        theta, _, anc, att = self.spec.transition.propose_device(
            B, self.prior, seed=self.seed, generation=self.gen, idx0=lo,
            max_attempts=self.sampler.max_attempts)
        # the prior log mass only for the rows kept (complete)
        return dict(theta=theta, lp=None, anc=anc), att

    def complete(self, got, att, unfiltered):
        if "lp" in got:
            return
        got["lp"] = self.prior.logpmf_rows(got["theta"])
        if unfiltered and att is not None:
            # rows kept unfiltered include proposals that exhausted
            # max_attempts: the proposal kernel's log mass for them is -inf
            gpu.mask_gave_up(got["lp"], att[:got["lp"].numel()],
                             self.sampler.max_attempts, -np.inf)


class _ModelsSource:
    """Candidate source of a generation over M > 1 models (one rank).  A
    round proposes (model, theta) per candidate (abc_models_propose: the
    reference's model steps and whole-attempt re-draw, smc.py:610-662) and
    simulates every row under its model; the kept rows are split by model at
    the end and weighted per model (smc.py:754-811):
    w = pi(m) prior_m(theta) / (model_factor(m) T_m(theta))."""

    def __init__(self, sampler, spec, seed, gen, dev, all_accepted):
        self.sampler, self.spec, self.dev = sampler, spec, dev
        self.seed, self.gen, self.all_accepted = seed, gen, all_accepted
        ms = self.ms = spec.models
        self.d = max(ms["d"])
        descs = []
        for m in range(ms["M"]):
            desc = dict(d=ms["d"][m], prior_kind=ms["prior_kind"][m],
                        prior_params=ms["prior_params"][m])
            tr = ms["transitions"][m]
            if tr is not None:
                desc.update(X=tr._dev_X, cdf=tr._dev_cdf, guide=tr._dev_guide, L=tr._dev_L)
            descs.append(desc)
        self.mset = gpu.ModelSet(descs, ms["model_cdf"], seed, gen, sampler.max_attempts)
        sims = [mod.fused_simulator(dev) if hasattr(mod, "fused_simulator") else None
                for mod in ms["vmodels"]]
        self.tables = None
        if all(sim is not None for sim in sims):
            self.tables = tuple(gpu.torch.stack([sim[k] for sim in sims]).contiguous()
                                for k in range(3))

    def propose(self, lo, B):
        model, theta, anc, att = self.mset.propose(lo, B)
        return dict(theta=theta, anc=anc, model=model), att

    def simulate(self, cand, lo):
        if self.tables is not None:
            return gpu.models_simulate_linear_gaussian(
                cand["theta"], cand["model"], *self.tables, self.seed, self.gen, lo)
        return self.sampler._simulate_by_model(
            self.ms, cand["model"], cand["theta"], self.seed, self.gen, lo,
            len(self.spec.sum_stat_keys))

    def kept_columns(self, cand):
        # model and ancestor travel as 8-byte columns of the one gather
        return dict(cand, model=cand["model"].to(gpu.I64))

    def complete(self, got, att, unfiltered):
        pass        # the prior density is taken per model (_assemble_models)

    def assemble(self, kept, led):
        cols = self.sampler._assemble_models(self.spec, kept, self.dev,
                                             self.all_accepted)
        return cols, None, dict(models=self.ms["M"],
                                accepted_per_model={m: len(c) for m, c in cols.items()})

    def sample(self, cols, recorded, record, ok, records):
        if recorded is None and cols:
            recorded = gpu.torch.cat([c.sum_stats for c in cols.values()])
        return ModelsSample(cols, recorded, self.spec.sum_stat_keys, record, ok)


class BatchedGPUSampler(Sampler):
    """Batched, device-resident sampler (nr_samples_per_param 1): fused or
    staged rounds for one model, staged rounds for 2 to 16 models.  The
    staged rounds are one loop over a candidate source (_OneModelSource,
    _ModelsSource), which proposes and simulates a round's candidates and
    turns the kept rows into the sample.  Closures outside that (a plain
    ``simulate_one``, a scalar model, ...) run the reference's per-candidate
    loop instead (_sample_per_candidate).

    Parameters
    ----------
    batch_size: candidates per rank and round (None: adapt to the measured
        acceptance rate).
    max_batch_size: cap on the adaptive batch of the staged path (default:
        what staged_round_bytes of candidate rows allow, at most 2^25).
    seed: base seed of the counter-based RNG (None: drawn from numpy's global
        RNG on rank 0 and broadcast).
    max_attempts: prior re-draws per candidate before giving up
        (the reference loops forever and warns at 1000, smc.py:658-662).
    check_max_eval: stop a generation once ``max_eval`` candidates are
        evaluated (sample not ok), like the reference samplers' flag of the
        same name (singlecore.py:14-26); off by default, as there.
    record_device_budget_bytes: optional cap on the HBM the recorded rows of
        one generation may take (default: none, as in the reference); when
        hit, the first rows that fit are kept and
        ``last_stats["records_truncated"]`` is set.
    """

    FUSED_MAX_STATS = 256     # abc_candidates_round: S <= SIM_SMAX
    FUSED_MAX_DIM = 64        # abc_candidates_round / _propose: d <= 64

    def __init__(self, batch_size=None, max_batch_size=None, seed=None,
                 max_attempts=10000, check_max_eval=False, fused=True,
                 max_fused_batch_size=1 << 31, filter_below=0.0,
                 filter_min_stats=5, record_budget_bytes=1 << 31,
                 record_device_budget_bytes=None, allow_per_candidate=True,
                 accept_tail=True):
        super().__init__()
        # a generation without a batched form (plain closure, non-vectorised
        # model, discrete host prior, ...) runs the per-candidate loop with a
        # warning; False makes it a TypeError instead
        self.allow_per_candidate = allow_per_candidate
        # the staged loop's one-pass accept tail (abc_pnorm_accept /
        # abc_aggregate_accept); False: the distance array and
        # abc_accept_compact, the same accepted rows
        self.accept_tail = accept_tail
        self.check_max_eval = check_max_eval
        self.batch_size = batch_size
        self.max_batch_size = max_batch_size
        # device bytes one staged round may hold in candidate rows (theta,
        # sum stats, distance, ancestor, the user simulator's output): at
        # low acceptance rounds of 2^22 candidates meant hundreds of rounds
        # (one host read each) per generation
        self.staged_round_bytes = 1 << 34
        self.seed = seed
        self.max_attempts = max_attempts
        # fused candidate rounds (abc_candidates_round): one kernel per round,
        # one accept bit per candidate, accepted rows regenerated; used when
        # the model is a LinearGaussianModel, the distance a PNormDistance,
        # the acceptor uniform and the transition an MVN / LocalTransition
        self.fused = fused
        self.max_fused_batch_size = max_fused_batch_size
        # early-reject mode (the lazy head: theta_0..3 and 4 statistics
        # decide most rejections) below this acceptance rate, for rounds
        # where the lazy head applies (_lazy_capable) with at least
        # filter_min_stats statistics.  Off by default: the round is bound
        # by the ancestor table's random accesses (~2 Infinity-Cache misses
        # per candidate, the same with or without the head) as much as by
        # its arithmetic, and the head rejects few candidates when the 4
        # statistics are a small part of the distance: c3 bench 4.54e6 vs
        # 4.78e6 accepted/s; tools/bench_fused.py 1.4e10 vs 1.9e10
        # candidates/s at S = 32 (profiles/r02_lazy_filter_ab.log,
        # r02_lazy_filter_S.log)
        self.filter_below = filter_below
        self.filter_min_stats = filter_min_stats
        self.record_budget_bytes = record_budget_bytes  # rec rows per fused round
        # first m recorded candidates are all that is used
        # (ABCSMC.max_nr_recorded_particles, smc.py:998-1001)
        self.max_nr_recorded = np.inf
        # optional cap on the HBM held by the recorded rows of one
        # generation (all ranks' rows in global order count).  Off by
        # default: the reference keeps every recorded row (smc.py:987-990),
        # and a cap would make the adaptive scales depend on the GPU memory
        # setting.  When set and hit, the first rows that fit are kept, as if
        # max_nr_recorded_particles had been set: logged, and
        # last_stats["records_truncated"] is True
        self.record_device_budget_bytes = record_device_budget_bytes
        self._acc_rate = None
        self._acc_trend = 1.0
        self.last_stats = {}
        # set by ABCSMC.run: host reads of the previous generation (its ESS
        # line), run once this generation's transition density is queued --
        # the longest kernel, so the host work overlaps it
        self.on_density_queued = None
        self._reader = _PinnedReader()     # the round's counts, one wait
        self._pool = (None, 0)             # (_kept_buffers' arena, offset)
        self._prop = (None, None, None)    # (spec, key, round) of _proposal_round

    def _base_seed(self, device):
        if self.seed is None:
            self.seed = dd.broadcast_int(np.random.randint(0, 2 ** 62), device)
        return self.seed

    def _round_size(self, needed, ws, d=1, S=1):
        if self.batch_size is not None:
            return int(self.batch_size)
        rate = self._acc_rate if self._acc_rate else 0.5
        # 30% margin: a second round costs more than the extra candidates
        b = int(math.ceil(needed / max(rate, 1e-9) * 1.3 / ws)) + 256
        cap = self.max_batch_size
        if cap is None:
            per = 8 * (2 * d + 2 * S) + 48     # theta, x (+ a user copy), dist, idx, lp, anc
            cap = max(1 << 16, min(1 << 25, self.staged_round_bytes // per))
        return int(min(max(b, 4096), cap))

    def sample_until_n_accepted(self, n, simulate_one, max_eval=np.inf,
                                all_accepted=False, show_progress=False):
        spec = simulate_one
        if not getattr(spec, "batched_capable", False):
            return self._sample_per_candidate(n, simulate_one, max_eval)
        dev = gpu.require_device()
        rank, ws = dd.world()
        seed = self._base_seed(dev)
        gen = spec.t & 0xFFFFFFFF
        record = self.sample_factory.record_rejected
        if getattr(spec, "models", None) is not None:
            src = _ModelsSource(self, spec, seed, gen, dev, all_accepted)
        elif getattr(spec, "grid", None) is not None:
            src = _GridSource(self, spec, seed, gen, dev, all_accepted)
        else:
            src = _OneModelSource(self, spec, seed, gen, dev, all_accepted)
            fr = None if all_accepted else self._fused_round(spec, seed, gen, dev)
            if fr is not None:
                return self._sample_fused(n, fr, spec, src, max_eval, record, dev,
                                          rank, ws)

        # staged rounds, the same loop for one model and for several: only
        # the candidate source differs
        S = len(spec.sum_stat_keys)
        kept = {k: [] for k in self._KEPT}       # kept rows' columns per round
        rec_x = []
        # no distance decides (calibration): every candidate is kept
        unfiltered = all_accepted or spec.distance is None
        stochastic = getattr(spec, "stochastic", None) is not None and not all_accepted
        # the accept tail (abc_pnorm_accept): a p-norm distance and the
        # uniform acceptor decided in one pass over the simulator's rows, no
        # distance array; the kept rows' distances afterwards
        tail = None
        if not (stochastic or unfiltered) and self.accept_tail:
            tail = self._accept_tail(spec, dev)
        # StochasticAcceptor + record_rejected: keep every evaluated
        # candidate's (theta, density, key, ancestor) for the temperature
        rec_extra = [] if (stochastic and record) else None
        led = self._ledger(n, rank, ws, S)
        while led.need > 0:
            if self.check_max_eval and led.n_eval >= max_eval:
                break
            B = self._limit_to_max_eval(self._round_size(led.need, ws, src.d, S),
                                        max_eval, led.n_eval, ws)
            kk = min(led.need, B)
            lo, _ = dd.rank_range(led.base, B, rank)
            cand, att = src.propose(lo, B)
            x = src.simulate(cand, lo)
            if x.dtype != gpu.F64 or not x.is_contiguous():
                # the kept-row gather moves 8-byte elements: every branch
                # below takes the simulator's rows as contiguous float64
                x = x.to(gpu.F64).contiguous()
            idx, cnt, dist, key, accw = self._accept(
                spec, x, att, kk, tail, unfiltered, stochastic, seed, gen, lo)
            cnt_local, pos = self._read_count(idx, cnt, kk, B, ws, unfiltered)
            counts = dd.allgather_counts(cnt_local, dev)
            k_mine, rec_rows = led.settle(counts, B, idx, pos, record)
            if k_mine:
                cols = dict(src.kept_columns(cand), x=x)
                if dist is not None:
                    cols["dist"] = dist
                if stochastic:
                    cols["w"] = accw
                got = dict(zip(cols, gpu.gather_rows_batch(list(cols.values()),
                                                           idx[:k_mine])))   # one launch
                if dist is None:
                    # the tail kept no distances: the kept rows' ones, the
                    # same per-row arithmetic (abc_pnorm / abc_aggregate_distance)
                    got["dist"] = tail.distances(got["x"], spec.x0vec)
                src.complete(got, att, unfiltered)
                for k, v in got.items():
                    kept[k].append(v)
            if record:
                # a pending multi-rank cut keeps the whole round's rows,
                # trimmed once the cutoff position is known (_finish)
                rr = B if rec_rows is None else rec_rows
                rec_x.append(x[:rr].clone() if rr < B // 2 else x[:rr])
                if rec_extra is not None:
                    anc = cand["anc"]
                    rec_extra.append((cand["theta"][:rr], dist[:rr], key[:rr],
                                      None if anc is None else anc[:rr]))
            self._acc_rate = max(int(counts.sum()) / float(ws * B), 1e-6)
        return self._finish(led, src, kept, rec_x if record else None, rec_extra, dev)

    def _accept(self, spec, x, att, kk, tail, unfiltered, stochastic, seed, gen, lo):
        """The accept step of one staged round over the rows x [B, S]:
        (idx, cnt, dist, key, accw) -- the accepted positions in candidate
        order and their number (cnt None when unfiltered: all B), the distance
        array (None with the tail), and the StochasticAcceptor's acceptance
        keys and weights (else None)."""
        B, dev = x.shape[0], x.device
        dist = cnt = key = accw = None
        if tail is not None:
            idx, cnt = tail.accept(x, spec.x0vec, spec.eps, kk, att=att,
                                   max_attempts=self.max_attempts)
        elif unfiltered:
            dist = gpu.torch.full((B,), np.inf, dtype=gpu.F64, device=dev)
            idx = gpu.torch.arange(B, dtype=gpu.I64, device=dev)
        else:
            dist = spec.distance.device_call(x, spec.x0vec, spec.t, spec.sum_stat_keys)
            # a proposal that exhausted max_attempts never enters the
            # population (the reference loops until the prior density is
            # positive, smc.py:649-662): its distance becomes NaN (never
            # <= eps, even at eps = inf); under a StochasticAcceptor the
            # "distance" is a density, so it becomes the zero-probability
            # density instead (acceptance 0, weight 0, and a zero
            # acceptance base in the temperature records)
            if att is not None:
                if stochastic:
                    gpu.mask_gave_up(dist, att, self.max_attempts,
                                     -np.inf if spec.stochastic[2] else 0.0)
                else:
                    gpu.mask_gave_up(dist, att, self.max_attempts)
            if stochastic:
                key, accw = gpu.stochastic_accept(dist, *spec.stochastic, seed, gen, lo)
                if att is not None:
                    # key +inf: never accepted, and marks the row for
                    # ABCSMC._device_records, which leaves it out
                    gpu.mask_gave_up(key, att, self.max_attempts, np.inf)
                idx, cnt = gpu.accept_compact(key, 0.0)
            else:
                idx, cnt = gpu.accept_compact(dist, spec.eps)
        return idx, cnt, dist, key, accw

    @staticmethod
    def _read_count(idx, cnt, kk, B, ws, unfiltered):
        """(this rank's accept count, the position of the kk-th accepted) of
        a staged round with at most one host read."""
        if unfiltered:
            # idx is arange(B): the k-th kept is candidate k - 1, no read
            return B, kk - 1
        if ws == 1:
            # one read: the count and the index of the n-th accepted
            # (meaningful only when this round completes the sample)
            nth = idx[kk - 1:kk] if idx.numel() >= kk else cnt.view(1)
            return gpu.torch.cat([cnt.view(1), nth]).cpu().tolist()
        return cnt, None          # gathered on the device, one host read

    @staticmethod
    def _simulate_by_model(ms, model, theta, seed, gen, lo, S):
        """User VectorizedModels: the round's rows are split by model
        (abc_models_partition), each model simulates its own rows [B_m, d_m]
        in one call and the statistics return to their rows.  The groups
        tile the round's index range (model m's rows take lo + offset_m ..),
        so every row keeps an index of its own within the generation."""
        torch = gpu.torch
        B = theta.shape[0]
        perm, counts = gpu.models_partition(model, ms["M"])
        x = torch.empty((B, S), dtype=gpu.F64, device=theta.device)
        off = 0
        for m, c in enumerate(counts.cpu().tolist()):
            if c == 0:
                continue
            sel = perm[off:off + c]
            th = gpu.gather_rows(theta, sel)[:, :ms["d"][m]].contiguous()
            xm = ms["vmodels"][m].simulate_batch(th, seed, gen, lo + off)
            x[sel] = xm.to(gpu.F64)
            off += c
        return x

    def _assemble_models(self, spec, kept, dev, all_accepted):
        """{m: ColumnarParticles} of the kept rows: split by model (stable,
        so every model's particles stay in candidate order) and weighted per
        model on its own segment."""
        torch = gpu.torch
        ms = spec.models
        if not kept["theta"]:
            return {}
        theta, x, anc, model, dist = (
            v[0] if len(v) == 1 else torch.cat(v)
            for v in (kept[k] for k in ("theta", "x", "anc", "model", "dist")))
        perm, counts = gpu.models_partition(model.to(torch.int32), ms["M"])
        out, off, queued = {}, 0, False
        for m, c in enumerate(counts.cpu().tolist()):
            if c == 0:
                continue
            th, xm, dm, am = gpu.gather_rows_batch([theta, x, dist, anc], perm[off:off + c])
            off += c
            th = th[:, :ms["d"][m]].contiguous()
            tr = ms["transitions"][m]
            if all_accepted or tr is None:
                # calibration, t = 0: w = n_acc / n_per_param = 1
                w = torch.ones(c, dtype=gpu.F64, device=dev)
            else:
                lp = gpu.prior_logpdf(th, ms["prior_kind"][m], ms["prior_params"][m])
                lt = tr.logpdf_device(th, hint=am)
                queued = True
                w = gpu.importance_weights(
                    lp, lt, spec.weight_scale * math.exp(ms["log_scale"][m]))
            out[m] = ColumnarParticles(th, w, dm.contiguous(), xm.contiguous(),
                                       ms["param_names"][m], spec.sum_stat_keys, m=m)
        if queued:
            # the previous generation's host reads, behind the densities
            hook, self.on_density_queued = self.on_density_queued, None
            if hook is not None:
                hook()
        return out

    @staticmethod
    def _accept_tail(spec, dev):
        """The distance's one-pass accept tail for this generation (an object
        with accept(...) and distances(rows, x0)), or None: a plain p-norm
        (abc_pnorm_accept) or an AggregatedDistance's term stack
        (abc_aggregate_accept)."""
        dist = spec.distance
        if hasattr(dist, "accept_tail"):
            return dist.accept_tail(spec.t, spec.sum_stat_keys, dev)
        if hasattr(dist, "fused_pnorm"):
            fp = dist.fused_pnorm(spec.t, spec.sum_stat_keys, dev)
            return None if fp is None else gpu.PNormTail(*fp)
        return None

    def _sample_per_candidate(self, n, simulate_one, max_eval):
        """A closure the batched kernels cannot run -- a plain
        ``simulate_one``, or a GenerationSpec whose model is not vectorised,
        whose distance or acceptor has no device form, ... (``why_not``) --
        goes through the reference's per-candidate loop
        (sampler/base.py:172-214, singlecore.py:20-38): candidates one at a
        time until n are accepted, each candidate's transition, prior and
        distance still calling the device kernels where they have them (a
        batch of one).  With several ranks rank 0 runs the loop and the
        sample is broadcast, so every rank holds the same population."""
        why = getattr(simulate_one, "why_not", "")
        if not self.allow_per_candidate:
            raise TypeError("BatchedGPUSampler: this generation has no batched "
                            "form (" + (why or type(simulate_one).__name__)
                            + ") and allow_per_candidate=False")
        logger.warning("BatchedGPUSampler: per-candidate loop, orders of "
                       "magnitude slower than the batched path (%s)",
                       why or type(simulate_one).__name__)
        rank, ws = dd.world()
        res = None
        if rank == 0:
            sample = self._create_empty_sample()
            n_eval = 0
            while sample.n_accepted < n:
                if self.check_max_eval and n_eval >= max_eval:
                    break
                particle = simulate_one()
                n_eval += 1
                sample.append(particle)
            if sample.n_accepted < n:
                sample.ok = False
            res = (sample, n_eval)
        sample, n_eval = dd.broadcast_object(res)
        self.nr_evaluations_ = int(n_eval)
        self.last_stats = dict(rounds=0, evaluations=int(n_eval),
                               accepted=int(sample.n_accepted), per_candidate=True)
        return sample

    # ---- fused candidate rounds ------------------------------------------
    def _fused_round(self, spec, seed, gen, dev):
        """gpu.CandidateRound of this generation, or None when some piece has
        no fused form (custom simulator / distance, stochastic acceptor)."""
        if not self.fused or getattr(spec, "stochastic", None) is not None \
                or spec.distance is None or len(spec.param_names) > self.FUSED_MAX_DIM:
            return None
        if getattr(spec, "grid", None) is not None:
            return None     # integer parameters: staged path (_GridSource)
        if spec.transition is None and getattr(spec, "host_prior", None):
            return None     # t = 0 draws of host-leg coordinates: staged path
        sim = (spec.model.fused_simulator(dev)
               if hasattr(spec.model, "fused_simulator") else None)
        fp = (spec.distance.fused_pnorm(spec.t, spec.sum_stat_keys, dev)
              if hasattr(spec.distance, "fused_pnorm") else None)
        if sim is None or fp is None or len(spec.sum_stat_keys) > self.FUSED_MAX_STATS:
            return None
        prop = {}
        if spec.transition is not None:
            arrays = getattr(spec.transition, "proposal_arrays", None)
            if arrays is None:
                return None
            prop = arrays()
        src, a, sigma = sim
        wf, pval = fp
        fr = gpu.CandidateRound(len(spec.param_names), len(spec.sum_stat_keys),
                                spec.prior_kind, spec.prior_params, src, a,
                                sigma, spec.x0vec, wf, pval, seed, gen,
                                self.max_attempts, **prop)
        fr.src_host = getattr(spec.model, "src", None)   # host copy (_lazy_capable)
        return fr

    LAZY_KT = 4              # abc_candidate.h: the lazy head's coordinates

    def _lazy_capable(self, spec, fr):
        """Whether the fused round's early reject can take the lazy head
        (abc_candidate.h lazy_filter_ok): shared Cholesky factor, d and S
        beyond the head, p in {1, 2, inf}, the first 4 statistics reading
        theta_0..3, and unbounded priors (norm, laplace), whose support
        holds every proposal; the kernel re-checks the bound exactly."""
        s = fr.spec
        kinds = getattr(spec, "prior_kind_host", None)
        src = getattr(fr, "src_host", None)
        return (s.X is not None and not s.per_particle_L and s.d > self.LAZY_KT
                and s.S >= max(5, self.filter_min_stats) and s.p in (1.0, 2.0, math.inf)
                and kinds is not None
                and all(k in (PRIOR_KINDS["norm"], PRIOR_KINDS["laplace"])
                        for k in kinds)
                and src is not None and all(0 <= int(v) < self.LAZY_KT for v in src[:4]))

    # candidates per rank a first round may spend on spare: about what one
    # more round costs in fixed time (launch, scan, host read and the
    # loop's host work, ~0.2 ms) at ~2e10 candidates/s
    FIRST_ROUND_SPARE = 4_000_000

    def _fused_size(self, need, ws, rate, measured, S, record):
        """Candidates per rank for the next fused round: need / rate, with a
        6% margin once the rate was measured in this generation, capped by
        the launch and record budgets.  The generation's first round takes
        the previous generation's rate times its last drop (eps shrinks, so
        the rate keeps falling) plus a spare of up to 10%, bounded by what a
        second round would cost: small early generations then finish in one
        round, large ones add little.  Round sizes never change the result
        (candidates are keyed by their global index; the first `need`
        accepted in index order are kept)."""
        if self.batch_size is not None:
            return int(self.batch_size)
        r = rate if rate else 0.5
        if measured:
            mult = 1.06
        else:
            r *= self._acc_trend if rate else 1.0
            mult = 1.0 + min(0.1, self.FIRST_ROUND_SPARE * ws * max(r, 1e-12) / max(need, 1))
        b = need / max(r, 1e-12) * mult / ws + 4096
        cap = self.max_fused_batch_size
        if record:
            cap = min(cap, max(self.record_budget_bytes // (8 * S), 4096))
        return int(min(max(b, 4096), cap))

    def _limit_to_max_eval(self, B, max_eval, n_eval, ws):
        """With check_max_eval no round goes past max_eval evaluations
        (singlecore.py:25-31 checks before every simulation; with several
        ranks the overshoot is below one candidate per rank)."""
        if not self.check_max_eval or not np.isfinite(max_eval):
            return B
        left = int(math.ceil(max_eval)) - int(n_eval)
        return int(max(1, min(B, left // ws)))

    def _ledger(self, n, rank, ws, S):
        return _RoundLedger(n, rank, ws, S, self.max_nr_recorded,
                            self.record_device_budget_bytes)

    def _sample_fused(self, n, fr, spec, src, max_eval, record, dev, rank, ws):
        """sample_until_n_accepted on fused rounds: per round one
        abc_candidates_round launch (accept bits -> indices of the first
        `need` accepted) and one host read; the kept rows are regenerated
        (abc_candidates_regen) bit-identical to the staged kernels."""
        torch = gpu.torch
        S = len(spec.sum_stat_keys)
        rec_x = []
        arena, arena_off = None, 0
        # kept rows: pooled buffers filled through raw addresses (one set of
        # views per buffer, built after the loop)
        kept, kept_off, kept_segs = None, 0, []
        row_bytes = (8 * fr.d, 8, 8, 8 * S, 8)
        led = self._ledger(n, rank, ws, S)
        rate, measured = self._acc_rate, False
        tot_B = tot_cnt = 0
        filtered = reruns = 0
        while led.need > 0:
            if self.check_max_eval and led.n_eval >= max_eval:
                break
            need = led.need
            B = self._limit_to_max_eval(self._fused_size(need, ws, rate, measured, S, record),
                                        max_eval, led.n_eval, ws)
            kk = min(need, B)
            lo, _ = dd.rank_range(led.base, B, rank)
            rx = None
            if record and led.rec_left > 0:
                # recorded rows of consecutive rounds land back to back in one
                # arena (the next round starts after the rows this one keeps),
                # so the generation's matrix is a view, not a concatenation
                if arena is None or arena_off + B > arena.shape[0]:
                    arena = torch.empty((int(B * 1.25) + 4096, S), dtype=gpu.F64, device=dev)
                    arena_off = 0
                rx = arena[arena_off:arena_off + B]
            filt = (rate is not None and rate < self.filter_below and rx is None
                    and self._lazy_capable(spec, fr))
            filtered += int(filt)
            # the generation's first round takes the threshold on the device
            # (queued behind the quantile kernel, no host wait); later rounds
            # the host value, which has arrived by then
            thr = getattr(spec, "eps_device", None) if led.rounds == 0 else None
            if thr is not None:
                idx, cnt = fr.run(lo, B, 0.0, cap=need, filter=filt, rec_x=rx,
                                  eps_dev=thr[0], eps_scale=thr[1])
            else:
                idx, cnt = fr.run(lo, B, spec.eps, cap=need, filter=filt, rec_x=rx)
            if ws == 1:
                # one read: the count and the index of the need-th accepted
                n_keep = cnt
                self._reader.queue(cnt, idx[kk - 1:kk])
            else:
                # several ranks: the round's counts are all-gathered on the
                # device and this rank's share of the first `need` accepted
                # (global order) is computed there, so the regeneration is
                # queued before any host read, as on one rank; the host reads
                # the gathered counts for its bookkeeping
                gathered = dd.allgather_counts_device(cnt)
                n_keep = gpu.round_keep(gathered, need, rank)
                self._reader.queue(gathered)
            # the kept rows' regeneration is queued before the count read,
            # sized on the device (the kept rows into the pooled buffer), so
            # the GPU is busy while the host reads the count
            if kept is None or kept_off + kk > kept[1]:
                if kept is not None and kept_off:
                    kept_segs.append((kept[0], kept_off))
                views = self._kept_buffers(kk, fr.d, S, dev)
                kept = (views, views[0].shape[0], [v.data_ptr() for v in views])
                kept_off = 0
            fr.regen_into(lo, idx.data_ptr(), kk,
                          [a + kept_off * b for a, b in zip(kept[2], row_bytes)],
                          n_dev=n_keep)
            counts = self._reader.wait()
            pos = None
            if ws == 1:
                counts, pos = counts[:1], int(counts[1])
            if thr is not None:
                spec.eps_device = None
                if np.isnan(thr[2].get()[0]):
                    # the select left the quantile undecided (knots in a tie
                    # run): the round ran at a NaN threshold and accepted
                    # nothing; run the same candidates again at the host
                    # value (the sort-based rerun, gpu.resolve_quantile).
                    # Every rank holds the same quantile, so all re-run
                    reruns += 1
                    continue
            k_mine, rr = led.settle(counts, B, idx, pos, rx is not None)
            kept_off += k_mine              # regenerated before the count read
            if rx is not None:
                # a pending multi-rank cut keeps the round whole (_finish trims)
                rec_x.append(rx if rr is None else rx[:rr])
                arena_off += rr or 0
            tot_B += ws * B
            tot_cnt += int(counts.sum())
            rate, measured = max(int(counts.sum()) / float(ws * B), 1e-12), True
        if kept is not None and kept_off:
            kept_segs.append((kept[0], kept_off))
        cols = {k: [] for k in self._KEPT}
        for views, cnt in kept_segs:
            th, lp, anc, x, dist = (v[:cnt] for v in views)
            for k, v in zip(("theta", "lp", "dist", "x", "anc"), (th, lp, dist, x, anc)):
                cols[k].append(v)
        new_rate = max(tot_cnt / float(max(tot_B, 1)), 1e-12)
        if self._acc_rate:
            self._acc_trend = min(1.0, max(0.5, new_rate / self._acc_rate))
        self._acc_rate = new_rate
        sample = self._finish(led, src, cols, rec_x if record else None, None, dev,
                              fused=True, candidates=int(tot_B),
                              filtered_rounds=filtered, quantile_reruns=reruns)
        if record and sample._recorded is None:
            # no round recorded a row: an empty matrix here
            sample._recorded = torch.empty((0, S), dtype=gpu.F64, device=dev)
        return sample

    _KEPT = ("theta", "lp", "dist", "x", "anc", "w", "model")  # columns of kept rows

    def _finish(self, led, src, kept, rec_x, rec_extra, dev, **stats):
        """The end of a generation, the same for every loop and source: the
        population from the kept rows (kept: lists of per-round pieces under
        _KEPT; src: the candidate source, which assembles them), the pending
        cut resolved and the last recorded pieces trimmed to it,
        nr_evaluations_ and last_stats (stats: the loop's own keys), the
        recorded rows (rec_x, rec_extra: this rank's pieces; None: the
        generation records nothing) and the sample."""
        cols, gathered, src_stats = src.assemble(kept, led)
        rr = led.finish(gathered)
        if rr is not None:
            rec_x[-1] = rec_x[-1][:rr]
            if rec_extra:
                rec_extra[-1] = tuple(None if a is None else a[:rr]
                                      for a in rec_extra[-1])
        self.nr_evaluations_ = int(led.n_eval)
        self.last_stats = dict(rounds=led.rounds, evaluations=int(led.n_eval),
                               accepted=int(led.n_acc), **src_stats, **stats,
                               records_truncated=led.records_truncated)
        recorded = records = None
        if rec_x is not None:
            recorded = self._gather_recorded(rec_x, led.rec_keeps, dev, led.ws)
            if rec_extra:
                records = tuple(
                    None if any(a is None for a in col)
                    else self._gather_recorded(list(col), led.rec_keeps, dev, led.ws)
                    for col in zip(*rec_extra))
        # (without record_rejected the source gives the population's statistics)
        return src.sample(cols, recorded, rec_x is not None, led.n_acc == led.n, records)

    # population columns of the fused rounds are carved from pooled device
    # arenas: a generation's new population (kept by the History) would
    # otherwise need fresh allocations -- a hipMalloc and its host stall --
    # every generation
    _POOL_BYTES = 1 << 28

    def _kept_buffers(self, cap, d, S, dev):
        """theta [cap, d], lp, anc (int64), x [cap, S], dist as views of one
        pooled fp64 arena."""
        torch = gpu.torch
        pieces = (((cap, d), cap * d), ((cap,), cap), ((cap,), cap),
                  ((cap, S), cap * S), ((cap,), cap))
        need = sum(n_el + (-n_el) % 32 for _, n_el in pieces)   # 256-byte aligned
        pool, off = self._pool
        if pool is None or pool.device != dev or off + need > pool.numel():
            pool = torch.empty(max(need, self._POOL_BYTES // 8), dtype=gpu.F64, device=dev)
            off = 0
        views = []
        for shape, n_el in pieces:
            views.append(pool[off:off + n_el].view(shape))
            off += n_el + (-n_el) % 32
        views[2] = views[2].view(torch.int64)
        self._pool = (pool, off)
        return tuple(views)

    def _gather_recorded(self, pieces, rec_keeps, dev, ws):
        """Concatenate this rank's recorded rows and, over several ranks,
        all-gather them back into global candidate-index order."""
        if not pieces:
            return None
        out = pieces[0] if len(pieces) == 1 else self._join_rows(pieces)
        if ws > 1:
            out = dd.allgather_rows_ordered([out.contiguous()], rec_keeps, dev)[0]
        return out.contiguous()

    @staticmethod
    def _join_rows(pieces):
        """Row blocks -> one [sum rows x S] tensor: a view when they lie back
        to back in one buffer (the fused rounds' record arena), else a copy."""
        torch = gpu.torch
        a = pieces[0]
        adjacent = all(
            p.dim() == 2 and p.is_contiguous() and p.shape[1] == a.shape[1]
            and p.untyped_storage().data_ptr() == a.untyped_storage().data_ptr()
            and p.data_ptr() == q.data_ptr() + q.numel() * q.element_size()
            for q, p in zip(pieces[:-1], pieces[1:]))
        if adjacent and a.is_contiguous():
            n = sum(p.shape[0] for p in pieces)
            return a.as_strided((n, a.shape[1]), a.stride())
        return torch.cat(pieces, 0)

    def _proposal_round(self, spec, seed, gen, dev):
        """A proposal-only gpu.CandidateRound of this generation (dummy
        simulator / distance fields, never read), cached per generation:
        the staged path's proposals through the fused kernel's propose_one
        (ancestor table, support box computed once per launch; the same bits
        as gpu.propose).  None when the transition has no proposal arrays."""
        # keyed on the spec object itself (held here, so its id cannot be
        # reused by a later run's spec while the entry lives)
        if len(spec.param_names) > self.FUSED_MAX_DIM:
            return None     # d > 64: the transition's own (wide) proposal kernel
        if getattr(spec, "grid", None) is not None:
            return None     # a grid prior has no device kinds (_GridSource)
        key = (seed, gen)
        if self._prop[0] is spec and self._prop[1] == key:
            return self._prop[2]
        arrays = None
        if spec.transition is not None:
            fn = getattr(spec.transition, "proposal_arrays", None)
            arrays = fn() if fn is not None else None
            if arrays is None:
                return None
        torch = gpu.torch
        z = torch.zeros(1, dtype=gpu.F64, device=dev)
        fr = gpu.CandidateRound(len(spec.param_names), 1, spec.prior_kind,
                                spec.prior_params, torch.zeros(1, dtype=torch.int32, device=dev),
                                z, z, z, z, 2.0, seed, gen, self.max_attempts,
                                **(arrays or {}))
        self._prop = (spec, key, fr)
        return fr

    def _propose(self, spec, B, seed, gen, lo, d):
        fr = None
        if not (spec.transition is None and getattr(spec, "host_prior", None)):
            fr = self._proposal_round(spec, seed, gen, gpu.require_device())
        if fr is not None:
            # the prior log-density only for the rows kept (computed after
            # the kept-row gather in sample_until_n_accepted)
            th, lp, anc, att = fr.propose(lo, B, with_lp=False)
            return th, lp, (anc if spec.transition is not None else None), att
        if spec.transition is None:
            th, lp, _, att = gpu.propose(None, None, None, spec.prior_kind,
                                         spec.prior_params, seed, gen, lo, B,
                                         self.max_attempts, d)
            anc = None
        else:
            th, lp, anc, att = spec.transition.propose_device(
                B, spec.prior_kind, spec.prior_params, seed=seed,
                generation=gen, idx0=lo, max_attempts=self.max_attempts)
        return th, lp, anc, att

    def _assemble(self, spec, kept, dev, d, all_accepted, led):
        """(population of the kept rows, weighted and gathered over the ranks
        in global order; the ranks' cutoff positions of a pending cut, else
        None).  kept: per-round pieces of the columns _KEPT."""
        torch = gpu.torch
        def cat(lst):
            if len(lst) == 1:
                return lst[0]
            if lst[0].dim() == 2:
                return self._join_rows(lst)
            return self._join_rows([t.view(-1, 1) for t in lst]).view(-1)
        rounds = len(kept["theta"])
        if rounds:
            theta, lp, dist, x = (cat(kept[k]) for k in ("theta", "lp", "dist", "x"))
        else:
            S = len(spec.sum_stat_keys)
            theta = torch.empty((0, d), dtype=gpu.F64, device=dev)
            lp = torch.empty(0, dtype=gpu.F64, device=dev)
            dist = torch.empty(0, dtype=gpu.F64, device=dev)
            x = torch.empty((0, S), dtype=gpu.F64, device=dev)
        # importance weights for this rank's accepted rows (smc.py:768-811);
        # a StochasticAcceptor's acceptance weights multiply in
        accw = cat(kept["w"]) if rounds and len(kept["w"]) == rounds else None
        if all_accepted:
            w = torch.ones(theta.shape[0], dtype=gpu.F64, device=dev)
        elif spec.transition is None:
            # t = 0: w = n_acc / n_per_param * prod(acceptance weights)
            w = (accw.contiguous() if accw is not None else
                 torch.ones(theta.shape[0], dtype=gpu.F64, device=dev))
        else:
            # ancestors of the accepted rows: population rows near them,
            # used by the x3 density kernel as exponent offsets
            anc = cat(kept["anc"]) if rounds and len(kept["anc"]) == rounds else None
            lt = spec.transition.logpdf_device(theta, hint=anc)
            hook, self.on_density_queued = self.on_density_queued, None
            if hook is not None:
                hook()
            hl = host_prior_logpdf(theta, getattr(spec, "host_prior", None))
            if hl is not None:
                lp = lp + hl      # the host-scipy leg's density factors
            w = gpu.importance_weights(lp, lt, spec.weight_scale,
                                       acc_w=None if accw is None else accw.contiguous())
        gathered = None       # the ranks' cutoff positions (_RoundLedger.finish)
        if led.ws > 1:
            # one packed all-gather; the rows come back in global
            # candidate-index order so the population (and every later draw
            # keyed on it) is the same for any number of ranks
            # (the cut rank's cutoff position rides in the same collective)
            parts = [theta, w, dist, x]
            extra = None if led.cut is None else led.cut["pos"]
            if len({a.dtype for a in parts}) == 1:
                got = dd.allgather_rows_ordered(parts, led.keeps, dev, extra=extra)
            else:
                got = [dd.allgather_rows_ordered([a], led.keeps, dev,
                                                 extra=extra if i == 0 else None)
                       for i, a in enumerate(parts)]
                if extra is not None:
                    got = ([got[0][0][0]] + [g[0] for g in got[1:]], got[0][1])
                else:
                    got = [g[0] for g in got]
            if extra is not None:
                got, gathered = got
            theta, w, dist, x = got
        if theta.shape[0] == 0:
            return None, gathered
        return ColumnarParticles(theta.contiguous(), w.contiguous(),
                                 dist.contiguous(), x.contiguous(),
                                 spec.param_names, spec.sum_stat_keys, m=0), gathered
