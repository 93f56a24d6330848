"""Epoch loops: the RawGnn branch (reference ``Helpers/TrainTestHelper.py:12-159``) and the Srrl branch (``:160-257``: KG steps, then the PS epoch).

Differences that do not change results: the running loss stays on the GPU and is read back once per epoch
(the reference syncs with ``loss.item()`` every step, ``TrainTestHelper.py:133``), and in a multi-process run
gradients are averaged across ranks by :class:`ihgnn_amd.distributed.GradientSync` before the optimiser step.
"""
import time
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
import torch.optim as optim

from ..Dataset import GraphDataset, TestSearchLogDataLoader
from .GlobalSettings import Gs
from .IOHelper import IOHelper
from .Metrics import Metrics
from .ProcessController import ProcessController


def print_network_parameters(module: nn.Module, name_filter: Optional[str] = None) -> None:
    rows = [(name, p) for name, p in module.named_parameters() if not name_filter or name_filter in name]
    if not rows:
        return
    shapes = ['(' + ', '.join(str(n) for n in p.size()) + ')' for _, p in rows]
    w_name, w_shape = max(len(n) for n, _ in rows), max(len(s) for s in shapes)
    with torch.no_grad():
        for (name, p), shape in zip(rows, shapes):
            grad = 'GRAD   ' if p.requires_grad else 'NO_GRAD'
            IOHelper.LogPrint(f'{name:<{w_name}} | size={shape:<{w_shape}} | {grad} | mean={p.mean().item():<7.3f} | '
                              f'std={p.std().item():<7.3f} | absmean={p.abs().mean().item():<7.3f}')


def seen_lists_for_logs(logs, indices, ptr, items) -> Tuple[List[int], List[int]]:
    """The items each of the logs ``indices`` is ranked WITHOUT under ``Gs.Evaluation.filter_seen``: its user's training items (run ``user`` of the lists
    ``(ptr, items)``, ``GraphDataset.user_item_lists``) except the log's own interacted items - a test positive that was also bought in training stays
    rankable, it is not turned into a guaranteed miss.  Returns ``(offsets [len(indices) + 1], flat item ids)``, each run ascending."""
    offsets, flat = [0], []
    for i in indices:
        user, _, interacted = logs[i][0], logs[i][1], logs[i][2]
        keep = set(int(x) for x in interacted)
        flat.extend(x for x in (int(v) for v in items[int(ptr[user]):int(ptr[user + 1])]) if x not in keep)
        offsets.append(len(flat))
    return offsets, flat


def sampled_candidate_set(index: int, own_items, item_count: int, count: int, seed: int = 0):
    """The set test log ``index`` is ranked among under ``Gs.Evaluation.sampled_candidates = count``: its own logged items plus ``count`` items drawn uniformly without
    replacement from the rest of the catalogue - int32, ascending.  The rule depends on the log's index alone, so every epoch, every rank and every chunking sees the
    same set: ``default_rng([seed, index])`` draws ``min(count + len(own), I)`` distinct ids in one call, the log's own are dropped from the draw and the first
    ``count`` of the rest are kept (all of them - the whole catalogue - when fewer remain)."""
    import numpy as np
    own = np.unique(np.asarray(own_items, np.int64))
    rng = np.random.default_rng([int(seed), int(index)])
    draw = rng.choice(int(item_count), size=min(int(count) + len(own), int(item_count)), replace=False, shuffle=False)
    drawn = draw[~np.isin(draw, own)][:int(count)]
    return np.union1d(own, drawn).astype(np.int32)


class SampledCandidates:
    """The sets of the logs ``indices`` as ONE CSR (``ptr`` int64 ``[len + 1]``, ``items`` int32, every run ascending: what ``ops.search_candidates`` takes as
    prepared), built once and kept beside the test logs (``for_loader``)."""

    def __init__(self, logs, indices, item_count: int, count: int, seed: int = 0):
        import numpy as np
        self.indices = np.asarray(list(indices), np.int64)
        runs = [sampled_candidate_set(int(i), logs[int(i)][2], item_count, count, seed) for i in self.indices]
        self.ptr = np.zeros(len(runs) + 1, np.int64)
        np.cumsum([len(r) for r in runs], out=self.ptr[1:])
        self.items = np.concatenate(runs).astype(np.int32) if runs else np.zeros(0, np.int32)
        self._position = {int(i): p for p, i in enumerate(self.indices.tolist())}

    def lists_for(self, part) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(offsets int64 [len(part) + 1], items int32)`` of the logs ``part``, in that order."""
        import numpy as np
        pos = np.asarray([self._position[int(i)] for i in part], np.int64)
        lengths = self.ptr[pos + 1] - self.ptr[pos]
        offsets = np.zeros(len(pos) + 1, np.int64)
        np.cumsum(lengths, out=offsets[1:])
        if len(pos) and np.array_equal(pos, np.arange(pos[0], pos[0] + len(pos))):      # a contiguous share: one slice
            flat = self.items[self.ptr[pos[0]]:self.ptr[pos[-1] + 1]]
        else:
            flat = np.concatenate([self.items[self.ptr[p]:self.ptr[p + 1]] for p in pos]) if len(pos) else np.zeros(0, np.int32)
        return torch.from_numpy(offsets), torch.from_numpy(np.ascontiguousarray(flat, np.int32))

    @staticmethod
    def for_loader(dataloader, indices, item_count: int, count: int, seed: int = 0) -> 'SampledCandidates':
        """The sets of this rank's share of ``dataloader.logs``, built at the first evaluation and reused by every later one."""
        key = (int(count), int(seed), int(item_count), len(indices), int(indices[0]) if len(indices) else -1)
        cached = getattr(dataloader, '_sampled_candidates', None)
        if cached is None or cached[0] != key:
            cached = (key, SampledCandidates(dataloader.logs, indices, item_count, count, seed))
            dataloader._sampled_candidates = cached
        return cached[1]


def _evaluate_batched(model, logs, item_count: int, device: torch.device, indices, seen=None, sampled: Optional[SampledCandidates] = None) -> List[Tuple[int, Metrics]]:
    """Top-10 of many searches per launch (``ihg_score_topk`` / ``ihg_score_topk_cosine``, whichever head ``Gs.Prediction.use_cosine_similarity`` names: scores on
    the matrix cores, running top-10 in registers, no ``[C, I]`` matrix), one D2H copy per chunk (the reference scores one log at a time and syncs on every one,
    ``TrainTestHelper.py:58-67``, ``Metrics.py:60-61``).  With ``Gs.Evaluation.extra_cutoffs`` the ONE ranking per chunk is as deep as the largest cutoff
    (``ihg_score_topk_deep``) and every cutoff's metrics are read from a prefix of it.  ``seen`` (``GraphDataset.user_item_lists`` under
    ``Gs.Evaluation.filter_seen``): every log is ranked without ``seen_lists_for_logs``' items, per-search lists built on the host per chunk.  ``sampled``
    (``Gs.Evaluation.sampled_candidates``): every log is ranked among ITS set only, by the list kernels (``top_items(..., candidate_lists=)``: the work is the sets'
    size, not the catalogue's); composes with ``seen``."""
    out: List[Tuple[int, Metrics]] = []
    chunk = 8192
    extras = tuple(Gs.Evaluation.extra_cutoffs)
    k = min(max((10,) + extras), item_count)
    for lo in range(0, len(indices), chunk):
        part = indices[lo:lo + chunk]
        uq = torch.tensor([(logs[i][0], logs[i][1]) for i in part], dtype=torch.long, device=device)
        if sampled is not None:
            exclude = None
            if seen is not None:
                offsets, flat = seen_lists_for_logs(logs, part, *seen)
                exclude = (torch.tensor(offsets, dtype=torch.int64), torch.tensor(flat, dtype=torch.int64))
            top = model.top_items(uq[:, 0], uq[:, 1], k, exclude=exclude, candidate_lists=sampled.lists_for(part))[0].tolist()
        elif seen is not None:
            offsets, flat = seen_lists_for_logs(logs, part, *seen)
            top = model.top_items(uq[:, 0], uq[:, 1], k, exclude=(torch.tensor(offsets, dtype=torch.int64), torch.tensor(flat, dtype=torch.int64)))[0].tolist()
        else:
            top = model.top_items(uq[:, 0], uq[:, 1], k)[0].tolist()      # HIP kernel: fp32-MFMA scores reduced to a running top-10 on chip
        for i, row in zip(part, top):
            _, _, items, flags, all_1 = logs[i]
            out.append((i, Metrics.at_cutoffs(row, items, flags, all_1, extras)))
    return out


def test_and_get_avg_metrics(model, dataset_train: GraphDataset, dataloader: TestSearchLogDataLoader,
                             get_long_tail_stat: bool = False) -> Tuple[Optional[List[Optional[Metrics]]], Metrics, float]:
    """-> (per-user average metrics or None, average over all usable logs, seconds).

    Logs are independent units: in a multi-process run each rank scores its contiguous share and the three metric sums
    and the count are all-reduced, so every rank returns the global average."""
    import torch.distributed as dist
    from .. import distributed as ihg_dist
    started = time.time()
    logs = dataloader.logs
    device = dataloader.device
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    mine = list(ihg_dist.shard_range(len(logs), rank, world))
    per_user: List[List[Metrics]] = [[] for _ in range(dataset_train.user_count)] if get_long_tail_stat else []
    total = Metrics()
    with torch.no_grad():
        model.save_features_for_test()
        try:
            if hasattr(model, 'top_items'):
                filtered = bool(Gs.Evaluation.filter_seen)
                drawn = int(Gs.Evaluation.sampled_candidates)
                if drawn < 0 or drawn >= dataset_train.item_count:
                    raise ValueError(f'Gs.Evaluation.sampled_candidates = {drawn}: 0 (off) or a count below the {dataset_train.item_count} items of the catalogue')
                sampled = SampledCandidates.for_loader(dataloader, mine, dataset_train.item_count, drawn, int(Gs.Evaluation.candidate_seed)) if drawn else None
                scored = _evaluate_batched(model, logs, dataset_train.item_count, device, mine, dataset_train.user_item_lists if filtered else None, sampled)
            else:
                scored = []
                for i in mine:
                    u, q, items, flags, all_1 = logs[i]
                    users = torch.tensor([u], device=device).expand(dataset_train.item_count)
                    queries = torch.tensor([q], device=device).expand(dataset_train.item_count)
                    scored.append((i, Metrics.calculate_on_all_items(model(users, queries, None), items, flags, all_1)))
        finally:
            model.clear_saved_feature()
    for i, m in scored:
        total.add_to_self(m)
        if get_long_tail_stat:
            per_user[logs[i][0]].append(m)
    extras = tuple(Gs.Evaluation.extra_cutoffs) if hasattr(model, 'top_items') else ()
    sums = ihg_dist.all_reduce_sums([total.HitRatio_at10, total.NDCG_at10, total.MAP_at10, float(len(scored))]
                                    + [v for cutoff in extras for v in total.extra.get(cutoff, (0.0, 0.0, 0.0))], device)
    counted = int(round(sums[3]))
    average = Metrics(sums[0], sums[1], sums[2], {cutoff: tuple(sums[4 + 3 * n:7 + 3 * n]) for n, cutoff in enumerate(extras)}).divide_and_get_new(max(counted, 1))
    user_avgs = None
    if get_long_tail_stat:                                  # per-user sums and counts, added up over the ranks' shares of the logs
        table = torch.zeros(dataset_train.user_count, 4, dtype=torch.float64)
        for user, ms in enumerate(per_user):
            for m in ms:
                table[user] += torch.tensor([m.HitRatio_at10, m.NDCG_at10, m.MAP_at10, 1.0], dtype=torch.float64)
        if world > 1:
            table = table.to(device)
            dist.all_reduce(table, op=dist.ReduceOp.SUM)
            table = table.cpu()
        user_avgs = [None if row[3] < 0.5 else Metrics(row[0], row[1], row[2]).divide_and_get_new(int(round(row[3])))
                     for row in table.tolist()]
    seconds = time.time() - started
    IOHelper.LogPrint(f'evaluation done in {seconds:<.2f} s over {counted} usable search logs' +
                      (f', each ranked among its own items and {int(Gs.Evaluation.sampled_candidates)} sampled ones' if hasattr(model, 'top_items') and Gs.Evaluation.sampled_candidates else '') +
                      (', each ranked without its user\'s training items.' if hasattr(model, 'top_items') and Gs.Evaluation.filter_seen else '.'))
    IOHelper.LogPrint(average.to_string(highlight=True), put_time_in_single_line=True)
    IOHelper.LogPrint()
    return user_avgs, average, seconds


# ``record_step='auto'``: an eager step faster than this is bound by the host's launch rate (config C1: 0.56 - 0.86 ms eager against 0.23 ms replayed; C2, 1.9 ms,
# gains nothing) - such a model is trained from a recorded step without being asked to
AUTO_RECORD_BELOW_MS = 1.5
_AUTO_WARM_STEPS, _AUTO_TIMED_STEPS = 3, 4


def _record_mode(record_step) -> str:
    if record_step in (True, 'on', '1', 'yes'):
        return 'on'
    if record_step in (False, 'off', '0', 'no'):
        return 'off'
    if record_step in (None, 'auto', ''):
        return 'auto'
    raise ValueError(f'record_step: on | off | auto, got {record_step!r}')


def log_clip_statistics(optimizer) -> None:
    """With gradient clipping on (``optimizer.max_grad_norm``): one line with the epoch's largest gradient norm and how many of its steps were scaled down - one host
    read of the three floats the clip launch keeps on the device.  Off: no line."""
    if getattr(optimizer, 'max_grad_norm', None) is None or not hasattr(optimizer, 'clip_statistics'):
        return
    largest, clipped, steps = optimizer.clip_statistics(reset=True)
    IOHelper.LogPrint(f'grad norm max {largest:<.4g} | clipped {clipped} of {steps} steps (max_grad_norm {optimizer.max_grad_norm:g})')


def srrl_kg_step(model, optimizer, batch, device: torch.device) -> torch.Tensor:
    """One KG step of the Srrl baseline (reference ``Helpers/TrainTestHelper.py:169-214``) on a batch of ``SrrlDatasetKG.collate_fn``; -> the loss (on the device)."""
    from .. import ops
    positive, negative, weight, mode, true_tail, true_head, true_query = batch
    positive, negative, weight = positive.to(device), negative.to(device), weight.to(device)
    true_tail, true_head, true_query = true_tail.to(device), true_head.to(device), true_query.to(device)
    optimizer.zero_grad()
    negative_score = model.trainkg((positive, negative, true_tail, true_head, true_query), mode=mode, positive_mode=False)
    positive_score = model.trainkg((positive, true_tail, true_head, true_query), mode=mode, positive_mode=True)
    loss = ops.kg_loss(positive_score.view(-1), negative_score, None if Gs.Srrl.uni_weight else weight)
    reported = loss.detach()
    if Gs.Srrl.regularization != 0.0:
        # as in the reference (TrainTestHelper.py:203-210) the term is formed from .weight.data: it changes the reported loss only and carries no gradient
        kg = model.KG
        squares = sum(t.weight.data.norm(p=2) ** 2 for t in (kg.embedding_user, kg.embedding_bag_vocabulary, kg.embedding_item))
        reported = reported + Gs.Srrl.regularization * (Gs.Srrl.regularization * squares)
    ops.backward(loss)
    optimizer.step()
    return reported


def srrl_ps_step(model, optimizer, batch, device: torch.device) -> torch.Tensor:
    """One PS step of the Srrl baseline (reference ``Helpers/TrainTestHelper.py:227-248``) on a batch of ``GraphDataset.collate_fn``; -> the loss (on the device)."""
    from .. import ops
    p_u, p_q, p_i, p_f, n_u, n_q, n_i, n_f = batch
    users, queries, items = (torch.cat(pair).to(device) for pair in ((p_u, n_u), (p_q, n_q), (p_i, n_i)))
    labels = torch.cat([p_f, n_f]).float().to(device)
    optimizer.zero_grad()
    loss = model.bce_loss(users, queries, items, labels)
    reported = loss.detach()
    if Gs.Srrl.regularization != 0.0:
        # (TrainTestHelper.py:237-244: from .weight.data as well - the reported loss only)
        squares = sum(t.weight.data.norm(p=2) ** 2 for t in (model.PS.embedding_user, model.KG.embedding_bag_vocabulary, model.PS.embedding_item))
        reported = reported + Gs.Srrl.regularization * (Gs.Srrl.regularization * squares)
    ops.backward(loss)
    optimizer.step()
    return reported


def train_srrl_and_get_avg_loss(model, optimizer, dataloader_train, pc: ProcessController, device: torch.device) -> Tuple[float, float]:
    """One epoch of the Srrl baseline (reference ``Helpers/TrainTestHelper.py:160-257``): ``model.srrl_steps`` KG steps from ``model.train_iterator_KG`` (under
    ``Gs.Srrl.KG_loss``), then the PS epoch over ``dataloader_train``; -> (average PS loss, seconds).  The losses stay on the device and are read once per phase."""
    started = time.time()
    model.train()
    if Gs.Srrl.KG_loss:
        kg_started = time.time()
        kg_sum = torch.zeros((), dtype=torch.float32, device=device)
        for _ in range(model.srrl_steps):
            kg_sum += srrl_kg_step(model, optimizer, model.train_iterator_KG.next(), device)
        IOHelper.LogPrint(f'[Epoch KG {pc.CurrentEpoch:<2d}] avg loss  KG->  {kg_sum.item() / max(model.srrl_steps, 1):<.4f} in {time.time() - kg_started:<.2f}s'
                          f' (remaining {pc.GetRemainingTimeString()}).')
    ps_started = time.time()
    ps_sum = torch.zeros((), dtype=torch.float32, device=device)
    batches = 0
    for batch in dataloader_train:
        ps_sum += srrl_ps_step(model, optimizer, batch, device)
        batches += 1
    avg_loss = ps_sum.item() / max(batches, 1)
    IOHelper.LogPrint(f'[Epoch PS {pc.CurrentEpoch:<2d}] avg loss {avg_loss:<.4f}  <-PS  in {time.time() - ps_started:<.2f}s (remaining {pc.GetRemainingTimeString()}).')
    log_clip_statistics(optimizer)                           # (the KG steps and the PS steps of the epoch together: one optimizer takes both)
    # (no learning-rate schedule: adjust_learning_rate is the RawGnn branch's, TrainTestHelper.py:155)
    return avg_loss, time.time() - started


def train_and_get_avg_loss(model, optimizer: optim.Optimizer, loss_function: nn.Module, dataset_train: GraphDataset,
                           dataloader_train, pc: ProcessController, device: torch.device,
                           grad_sync=None, record_step='auto') -> Tuple[float, float]:
    """One epoch over ``dataloader_train`` -> (average loss, seconds) - the reference's loop (``Helpers/TrainTestHelper.py:123-143``).  ``record_step`` (single
    process, fused loss, the HIP Adam): batches of the common size run as replays of ONE recorded step (``ihgnn_amd.captured_step``: worth it where the step is
    bound by the host's launch rate, i.e. on small graphs); other batch sizes - the epoch's last batch - run eagerly.  ``'auto'`` (default): the first steps of the
    first epoch run eagerly, steps 4 - 7 are timed, and the step is recorded when they took less than ``AUTO_RECORD_BELOW_MS`` each; ``'on'`` / ``'off'`` decide
    without measuring.  A model the recording refuses (a parameter without gradient) trains eagerly, with one log line.

    The objective of every step is ``ops.training_objective``'s (the settings ``--loss`` and ``--hard_negatives M`` write): a step is ``model.training_loss`` where the
    fused batch tail runs; where it does not, ``ops.objective_loss`` on the model's scores under an objective over groups (a ranking loss of every positive against
    its own negatives, or any loss over the best of a pool of M candidates: ``loss_function`` and the labels are then not used) and ``loss_function`` otherwise."""
    from ..Models.Srrl import Srrl
    if isinstance(model, Srrl):
        if grad_sync is not None or _record_mode(record_step) == 'on':
            raise NotImplementedError('the Srrl baseline trains in one process, eagerly: no gradient exchange, no recorded step')
        return train_srrl_and_get_avg_loss(model, optimizer, dataloader_train, pc, device)
    started = time.time()
    loss_sum = torch.zeros((), dtype=torch.float32, device=device)
    batches = positives = 0
    sampler = getattr(dataloader_train, 'batch_sampler', None)
    if hasattr(sampler, 'set_epoch'):
        sampler.set_epoch(pc.CurrentEpoch)                  # data parallel: a fresh shared permutation per epoch (ShardedBatchSampler)
    mode = _record_mode(record_step)
    from .. import ops
    from ..optim import Adam as _HipAdam
    can_record = mode != 'off' and grad_sync is None and device.type == 'cuda' and isinstance(optimizer, _HipAdam)
    decision = getattr(model, '_record_decision', None) if can_record else False       # None: undecided (auto, still measuring); True / False
    if can_record and mode == 'on' and decision is not True and not getattr(model, '_record_refused', False):
        # an explicit 'on' overrides what an earlier 'auto' epoch measured (False = "not launch-bound"); only a REFUSED recording (the capture raised) stays off
        decision = model._record_decision = True
    if decision and getattr(model, '_recorded_step', None) is not None and model._recorded_step.stale(full=True):
        model._recorded_step = None                          # an IHG_* switch or ops flag changed since the recording (checked once per epoch; the per-step check is the cheap one)
    eager_seen, timed_from = getattr(model, '_auto_eager_steps', 0), None      # (persist across epochs: an epoch may be shorter than the measurement)
    for p_u, p_q, p_i, p_f, n_u, n_q, n_i, n_f in dataloader_train:
        positives += len(p_u)
        users, queries, items = torch.cat([p_u, n_u]), torch.cat([p_q, n_q]), torch.cat([p_i, n_i])
        flags = torch.cat([p_f, n_f]).float()
        objective = ops.training_objective(len(users), len(p_u))      # the settings are read per step, as the model reads its head; grouped: no labels, no loss_function
        if objective.grouped:
            fused = getattr(model, 'supports_fused_tail', None) and model.supports_fused_tail()
        else:
            fused = getattr(model, 'supports_fused_loss', None) and model.supports_fused_loss(loss_function)
        if decision and fused:
            recorded = getattr(model, '_recorded_step', None)
            if recorded is None or recorded.optimizer is not optimizer or recorded.stale():     # (stale: a hyper-parameter baked into the recording changed)
                from ..captured_step import CapturedTrainingStep
                try:
                    recorded = model._recorded_step = CapturedTrainingStep(model, optimizer, int(users.shape[0]), warmup_batch=(users, queries, items, flags),
                                                                                  positives=objective.positives)
                except (ValueError, RuntimeError) as refused:
                    # ValueError: the recording's own refusal (a parameter without gradient, ...); RuntimeError: the stream capture failed (an op that synchronises,
                    # an allocation the capture cannot hold) - under 'auto' nobody asked for a recording, so either way the run goes on eagerly; under 'on' a
                    # capture failure is the caller's to see
                    if mode == 'on' and isinstance(refused, RuntimeError):
                        raise
                    IOHelper.LogPrint(f'training step not recorded ({type(refused).__name__}: {refused}); training eagerly')
                    recorded, decision = None, False
                    model._recorded_step, model._record_decision, model._record_refused = None, False, True
                    optimizer.zero_grad(set_to_none=True)
            if recorded is not None and recorded.batch_rows == int(users.shape[0]) and (not objective.grouped or recorded.positives == objective.positives):
                loss_sum += recorded.step(users, queries, items, flags, positives=len(p_u))
                batches += 1
                continue
        # auto: a few eager steps are timed (the step alone, device drained on both sides - not the loader's work between steps) once the allocator and the workspaces are warm
        time_this = decision is None and fused and _AUTO_WARM_STEPS <= eager_seen < _AUTO_WARM_STEPS + _AUTO_TIMED_STEPS
        if time_this:
            torch.cuda.synchronize(device)
            timed_from = time.perf_counter()
        if getattr(model, '_recorded_step', None) is not None:
            optimizer.zero_grad(set_to_none=True)           # the last replay's gradients (in the recording's pool) must not be accumulated onto
        cotangent = getattr(grad_sync, 'mode', None) == 'cotangent'
        if cotangent and not fused:
            raise RuntimeError('--grad_sync cotangent exchanges the fused batch tail\'s row gradients: it needs the HIP model and a plain BCEWithLogitsLoss (use bucketed / sharded)')
        if fused:
            loss = model.training_loss(users, queries, items, objective, flags, cotangent_sync=grad_sync if cotangent else None)
        elif objective.grouped:
            loss = ops.objective_loss(model(users, queries, items), objective)
        else:
            loss = loss_function(model(users, queries, items), flags)
        loss_sum += loss.detach()
        if loss.is_cuda:
            ops.backward(loss)                               # loss.backward() with a cached root gradient (no fill launch per step)
        else:
            loss.backward()
        if grad_sync is not None:
            grad_sync.average_gradients()
        optimizer.step()
        if grad_sync is not None:
            grad_sync.zero_grad()           # keeps the .grad views into the flat all-reduce buffer
        else:
            optimizer.zero_grad()
        batches += 1
        if decision is None and fused:
            if time_this:
                torch.cuda.synchronize(device)
                model._auto_timed_seconds = getattr(model, '_auto_timed_seconds', 0.0) + (time.perf_counter() - timed_from)
            eager_seen += 1
            model._auto_eager_steps = eager_seen
            if eager_seen == _AUTO_WARM_STEPS + _AUTO_TIMED_STEPS:
                step_ms = model._auto_timed_seconds * 1e3 / _AUTO_TIMED_STEPS
                decision = model._record_decision = bool(step_ms < AUTO_RECORD_BELOW_MS)
                model._auto_step_ms = step_ms
                IOHelper.LogPrint(f'eager training step {step_ms:.2f} ms: ' + ('launch-bound - from here on ONE recorded step (hipGraph) is replayed' if decision
                                                                              else 'GPU-bound - steps stay eager'))
    avg_loss = loss_sum.item() / max(batches, 1)
    if getattr(grad_sync, 'mode', None) == 'cotangent' and grad_sync.world_size > 1:
        # the cotangent exchange never moves a parameter or a dense gradient between the ranks: the replicas stay identical because every rank takes the same deterministic
        # step.  Once per epoch that is CHECKED (one broadcast of the parameters); a drift - a non-deterministic kernel, a rank that skipped a step - is reported and
        # healed from rank 0 instead of growing silently
        drift = grad_sync.check_replicas()
        if drift != 0.0:
            IOHelper.LogPrint(f'WARNING: replicas drifted apart under --grad_sync cotangent (largest parameter difference {drift:.3e}); re-broadcasting rank 0\'s parameters')
            grad_sync.broadcast_parameters(0)
    if grad_sync is not None and grad_sync.world_size > 1:  # every rank reports (and schedules its learning rate on) the global average
        from .. import distributed as ihg_dist
        total, count = ihg_dist.all_reduce_sums([avg_loss * batches, float(batches)], device)
        avg_loss = total / max(count, 1.0)
    seconds = time.time() - started
    IOHelper.LogPrint(f'[Epoch \033[0;44m{pc.CurrentEpoch:>2d}/{pc.EndEpoch - 1}\033[0m] average loss '
                      f'\033[0;45m{avg_loss:<.4f}\033[0m on {positives} interactions in {seconds:<.2f} s '
                      f'(remaining {pc.GetRemainingTimeString()}).')
    log_clip_statistics(optimizer)
    if Gs.adjust_learning_rate and avg_loss < 0.008 and Gs.learning_rate > 0.0004:
        Gs.learning_rate *= 0.98
        for group in optimizer.param_groups:
            group['lr'] = Gs.learning_rate
        IOHelper.LogPrint(f'learning rate -> {Gs.learning_rate}')
    return avg_loss, seconds
