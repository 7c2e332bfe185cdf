"""Device-resident clip store on the MI355X: a draw is gather + DevicePreStep bit for bit, the epoch's bookkeeping, capture, offsets
past 2 and 4 GiB, the trainer's step_from against step(), and the sampler glue."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

from oracle import prestep_oracle as PO

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MASK = (0, 7, 8, 9)
P = 104
STEP = 8.0          # the random walks' step: large against the spread of the centres, so that the velocity blocks decide labels


def _walk(rng, n, width):
  """A random walk with large steps, as tests/test_prestep.py::_inputs builds its poses."""
  x = np.empty((n, width), dtype=np.float32)
  x[0] = rng.standard_normal(width) * 40 + 100
  x[1:] = x[0] + np.cumsum(rng.standard_normal((n - 1, width)) * STEP, axis=0)
  return x


def _stats(rng, F):
  """The statistics of tests/test_prestep.py::_inputs, with its var == 0 and var < 0 columns."""
  pose_mean, pose_var = rng.standard_normal(P) * 10 + 100, rng.random(P) * 50 + 1
  pose_var[5] = 0.0
  pose_var[11] = -1e-9
  audio_mean, audio_var = rng.standard_normal(F), rng.random(F) * 4 + 0.1
  return pose_mean, pose_var, audio_mean, audio_var


def _centers(rng, M, PK, feats):
  """Centres whose pose blocks lie close together and whose velocity / speed blocks are as wide as the walks' steps."""
  blocks = {'pose': rng.standard_normal((M, PK)) + 100, 'velocity': rng.standard_normal((M, PK)) * STEP,
            'speed': np.abs(rng.standard_normal((M, PK // 2))) * STEP * 1.25}
  return np.concatenate([blocks[f] for f in feats], axis=1)


@functools.lru_cache(maxsize=None)
def _dataset(lengths, F, M, feats, mask=MASK, seed=5, n_styles=5):
  rng = np.random.default_rng(seed)
  intervals = [(_walk(rng, n, P), (rng.standard_normal((n, F)) * 3 - 20).astype(np.float32), 3 + i % n_styles) for i, n in enumerate(lengths)]
  PK = P - 2 * len(mask)
  return intervals, _centers(rng, M, PK, feats), _stats(rng, F)


def _store_and_pre(lengths, F, M, feats, T, hop, mask=MASK, **kw):
  from mix_stage_amd import DeviceClipStore, DevicePreStep
  intervals, centers, stats = _dataset(tuple(lengths), F, M, tuple(feats), tuple(mask))
  pre = DevicePreStep(centers, *stats, mask=mask, feats=feats, device=DEV)
  store = DeviceClipStore([(torch.from_numpy(p), torch.from_numpy(a), s) for p, a, s in intervals], T=T, hop=hop, device=DEV, **kw)
  return store, pre, intervals, centers


def _znorm_full(pre, pose):
  """ms_znorm_select with keep = NULL: the z-normed full pose."""
  from mix_stage_amd._lib import check, lib
  pose = pose.contiguous()
  out = torch.empty_like(pose)
  vp = lambda t: ctypes.c_void_p(t.data_ptr())
  check(lib().ms_znorm_select(vp(pose), None, vp(pre.pose_mean), vp(pre.pose_inv), vp(out), pose.shape[0] * pose.shape[1], pre.P, pre.P,
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'ms_znorm_select')
  return out


def _reference(store, pre, ids):
  """Gather the windows `ids` with torch, then DevicePreStep.__call__: (audio, labels, y, style, full)."""
  ids = torch.as_tensor(ids, dtype=torch.int64)
  rows = (torch.tensor(store.row_start)[store.win_interval[ids]] + store.win_start[ids])[:, None] + torch.arange(store.T)[None, :]
  rows = rows.to(DEV)
  pose, audio = store.pose_rows[rows], store.audio_rows[rows]
  a, labels, y = pre(pose, audio)
  style = torch.tensor(store.styles)[store.win_interval[ids]].to(DEV)[:, None].expand(-1, store.T).contiguous()
  return a, labels, y, style, _znorm_full(pre, pose)


def _assert_draw(got, ref):
  names = ('audio', 'labels', 'y', 'style', 'pose_full_norm')
  for name, g, r in zip(names, got, ref):
    assert g.dtype == r.dtype and g.shape == r.shape, name
    assert torch.equal(g, r), name


# ---- 1. draw == gather + DevicePreStep -------------------------------------------------------------------------
LENGTHS = (64, 65, 130, 63, 200)
PV, PVS = ('pose', 'velocity'), ('pose', 'velocity', 'speed')
CASES = [(F, M, feats, 64, 7) for F, M, feats in itertools.product((128, 5), (1, 5), (PV, PVS))] + [(128, 5, PVS, 32, 3)]


def _first_frame_pitfall_visible(store, intervals, centers, feats, order):
  """On the CPU, with the oracle: some drawn window starts behind its interval's first row, and for those windows the labels that
  take the velocity at t = 0 from the preceding row differ from the correct ones somewhere.  (With M = 1 every label is 0: such a
  case cannot see the pitfall, and the assertion on the labels is made for M > 1 only.)"""
  inside, differ = 0, 0
  for w in order:
    i, s = int(store.win_interval[w]), int(store.win_start[w])
    if s == 0:
      continue
    inside += 1
    pose = intervals[i][0]
    good = PO.kmeans_predict(PO.remove_joints(pose[None, s:s + store.T], MASK), centers, feats)[0]
    leaky = PO.kmeans_predict(PO.remove_joints(pose[None, s - 1:s + store.T], MASK), centers, feats)[0, 1:]
    differ += int((good != leaky).sum())
  return inside, differ


@pytest.mark.parametrize('F,M,feats,T,hop', CASES, ids=lambda v: '+'.join(v) if isinstance(v, tuple) else str(v))
def test_draw_is_gather_plus_prestep_bit_for_bit(F, M, feats, T, hop):
  B = 3
  store, pre, intervals, centers = _store_and_pre(LENGTHS, F, M, feats, T, hop, batch_size=B)
  store.new_epoch()
  from mix_stage_amd.clip_store import epoch_order
  order = epoch_order(store.W, 0, 0)
  steps = store.steps_left
  assert steps == store.W // B and steps >= 2
  inside, differ = _first_frame_pitfall_visible(store, intervals, centers, feats, order[:steps * B].tolist())
  assert inside > 0
  if M > 1:
    assert differ > 0, 'the input cannot see a velocity taken from the row in front of a window'
  for i in range(steps):
    got = store.draw(pre, B, full_pose=True)
    ids = order[i * B:(i + 1) * B]
    assert torch.equal(store.last_indices.cpu(), ids)
    _assert_draw(got, _reference(store, pre, ids))
  assert store.steps_left == 0
  store.check()


# ---- 2. epoch bookkeeping ----------------------------------------------------------------------------------------
def test_epoch_bookkeeping_and_device_guard():
  from mix_stage_amd.clip_store import epoch_order
  B = 3
  store, pre, _, _ = _store_and_pre((83, 83), 5, 5, PV, 64, 1, seed=11, batch_size=B)
  twin, _, _, _ = _store_and_pre((83, 83), 5, 5, PV, 64, 1, seed=11, batch_size=B)
  assert store.W == 40
  store.new_epoch()
  twin.new_epoch()
  order0 = epoch_order(40, 11, 0)
  seen = []
  for i in range(13):
    store.draw(pre, B)
    assert torch.equal(store.last_indices.cpu(), order0[3 * i:3 * i + 3])
    seen.extend(store.last_indices.tolist())
  assert len(set(seen)) == 39 and store.steps_left == 0
  with pytest.raises(IndexError):
    store.draw(pre, B)
  assert store.state()['cursor'] == 39                          # the refused draw launched nothing
  assert torch.equal(store.state()['order'], twin.state()['order']) and torch.equal(twin.state()['order'], order0)
  store.new_epoch()
  twin.new_epoch()
  order1 = store.state()['order']
  assert not torch.equal(order1, order0) and torch.equal(order1, twin.state()['order']) and torch.equal(order1, epoch_order(40, 11, 1))
  assert store.state()['cursor'] == 0 and store.steps_left == 13
  # a caller's order of 7 entries: 2 steps
  mine = [5, 39, 0, 17, 21, 8, 30]
  store.new_epoch(mine)
  assert store.steps_left == 2
  for i in range(2):
    store.draw(pre, B)
    assert store.last_indices.tolist() == mine[3 * i:3 * i + 3]
  with pytest.raises(IndexError):
    store.draw(pre, B)
  # the device guard: one draw through the unchecked entry point at cursor 6 -- position 6 is real, 7 and 8 are "no window"
  got = store.draw(pre, B, full_pose=True, _unchecked=True)
  assert store.last_indices.tolist() == [30, -1, -1]
  ref = _reference(store, pre, [30])
  for g, r in zip(got, ref):
    assert torch.equal(g[:1], r)
    assert g[1:].numel() > 0 and not g[1:].any()                # zeros, label 0, style 0 (the store's style ids start at 3)
  assert ref[3].min() >= 3
  with pytest.raises(RuntimeError):
    store.check()
  store.new_epoch()
  store.check()
  # state() / set_state(): a twin resumed in the middle of an epoch draws what the store draws
  store.draw(pre, B)
  twin.set_state(store.state())
  assert twin.steps_left == store.steps_left == 12
  a, b = store.draw(pre, B), twin.draw(pre, B)
  assert torch.equal(store.last_indices, twin.last_indices)
  _assert_draw(a, b)



def test_two_ranks_draw_disjoint_halves_of_every_step():
  """The device arithmetic of sharding: two stores of one set as rank 0 and rank 1 of a world of 2, on one GPU.  Rank r's clip b of
  a step is window order[cursor + r * B + b], the cursor moves by world * B, and the epoch holds W // (world * B) steps."""
  from mix_stage_amd.clip_store import epoch_order
  B, world = 3, 2
  made = [_store_and_pre(LENGTHS, 128, 5, PVS, 64, 7, rank=r, world=world, batch_size=B) for r in range(world)]
  stores, pre = [m[0] for m in made], made[0][1]
  order = epoch_order(stores[0].W, 0, 0)
  for st in stores:
    st.new_epoch()
    assert st.steps_left == st.W // (world * B) == 5
    assert torch.equal(st.state()['order'], order)
  seen = []
  for i in range(5):
    for r, st in enumerate(stores):
      got = st.draw(pre, B, full_pose=True)
      ids = order[i * world * B + r * B:i * world * B + (r + 1) * B]
      assert torch.equal(st.last_indices.cpu(), ids)
      _assert_draw(got, _reference(st, pre, ids))
      assert st.state()['cursor'] == (i + 1) * world * B
      seen.extend(ids.tolist())
  assert sorted(seen) == sorted(order[:30].tolist()) and len(set(seen)) == 30
  for st in stores:
    assert st.steps_left == 0
    with pytest.raises(IndexError):
      st.draw(pre, B)
    st.check()


# ---- 3. capture --------------------------------------------------------------------------------------------------
def test_captured_draw_replays_through_the_order():
  B = 3
  store, pre, _, _ = _store_and_pre(LENGTHS, 128, 5, PVS, 64, 7)
  twin, _, _, _ = _store_and_pre(LENGTHS, 128, 5, PVS, 64, 7)
  store.new_epoch()
  twin.new_epoch()
  warm, _, _, _ = _store_and_pre(LENGTHS, 128, 5, PVS, 64, 7)
  warm.new_epoch()
  warm.draw(pre, B, full_pose=True)                           # (the kernels' first launches in this process: not inside a capture)
  bufs = [torch.zeros((B, 64, 128), device=DEV), torch.zeros((B, 64), dtype=torch.int64, device=DEV),
          torch.zeros((B, 64, pre.PK), device=DEV), torch.zeros((B, 64), dtype=torch.int64, device=DEV), torch.zeros((B, 64, P), device=DEV)]
  torch.cuda.synchronize()
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    store.draw_into(pre, *bufs[:4], full=bufs[4])
  assert store.state()['cursor'] == 0                         # the capture ran nothing
  for i in range(4):
    g.replay()
    got = [b.clone() for b in bufs]
    idx = store._indices[:B].clone()
    ref = twin.draw(pre, B, full_pose=True)
    _assert_draw(got, ref)
    assert torch.equal(idx, twin.last_indices)
  assert store.state()['cursor'] == 4 * B
  store.mark_drawn(B, 4)
  assert store.steps_left == twin.steps_left
  store.check()


# ---- 4. offsets past 2 GiB and 4 GiB -----------------------------------------------------------------------------
def test_rows_past_2_and_4_gib():
  from mix_stage_amd import DeviceClipStore, DevicePreStep
  R, F, T = 10_400_000, 128, 64
  pose_rows = torch.zeros((R, P), device=DEV)                 # 4.3 GB
  audio_rows = torch.zeros((R, F), device=DEV)                # 5.3 GB
  mid = 2 ** 31 // (P * 4) + 1                                # the first row that lies wholly past byte 2^31 of the pose store
  assert mid * P * 4 > 2 ** 31 and (R - T) * P * 4 > 2 ** 32 and (R - T) * F * 4 > 2 ** 32
  starts = [0, mid, R - T]
  lengths = [T, mid - T, T, R - T - (mid + T), T]
  assert sum(lengths) == R
  rng = np.random.default_rng(9)
  centers, stats = _centers(rng, 5, 96, PVS), _stats(rng, F)
  slices = []
  for s in starts:
    pose = torch.from_numpy(_walk(rng, T, P)).to(DEV)
    audio = torch.from_numpy((rng.standard_normal((T, F)) * 3 - 20).astype(np.float32)).to(DEV)
    pose_rows[s:s + T] = pose
    audio_rows[s:s + T] = audio
    slices.append((pose, audio))
  store = DeviceClipStore.from_rows(pose_rows, audio_rows, lengths, [3, 4, 5, 6, 7], T=T, hop=T)
  pre = DevicePreStep(centers, *stats, mask=MASK, feats=PVS, device=DEV)
  ids = [int((store.win_interval == i).nonzero()[0]) for i in (0, 2, 4)]
  assert [int(store.win_start[w]) for w in ids] == [0, 0, 0]
  store.new_epoch(ids)
  got = store.draw(pre, 3, full_pose=True)
  assert store.last_indices.tolist() == ids
  pose = torch.stack([p for p, _ in slices])
  a, labels, y = pre(pose, torch.stack([a for _, a in slices]))
  style = torch.tensor([3, 5, 7], device=DEV)[:, None].expand(-1, T).contiguous()
  _assert_draw(got, (a, labels, y, style, _znorm_full(pre, pose)))
  assert len(set(labels.flatten().tolist())) > 1 and bool(a.any())
  store.check()


# ---- 5. trainer --------------------------------------------------------------------------------------------------
def _trainer_set():
  rng = np.random.default_rng(21)
  lengths = (70, 90, 74, 83, 77, 88)
  intervals = [(torch.from_numpy(_walk(rng, n, P)), torch.from_numpy(rng.standard_normal((n, 128)).astype(np.float32)), i % 2)
               for i, n in enumerate(lengths)]
  rows = torch.cat([p for p, _, _ in intervals]).double()
  arows = torch.cat([a for _, a, _ in intervals]).double()
  centers = _centers(rng, 2, P, PV)
  stats = (rows.mean(0).numpy(), rows.var(0, unbiased=False).numpy(), arows.mean(0).numpy(), arows.var(0, unbiased=False).numpy())
  return intervals, centers, stats


@pytest.fixture
def trainer_globals_restored():
  """MixStageTrainStep switches the trainer's process-wide modes on (prepared weights, deferred weight gradients): off again for the
  tests that run after this file."""
  from mix_stage_amd import ops
  yield
  ops.enable_prepared_weights(False)
  ops.enable_deferred_wgrad(False)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_step_from_is_step_on_the_drawn_batch(dtype, trainer_globals_restored):
  import mix_stage_amd as A
  from mix_stage_amd.train_step import MixStageTrainStep
  from test_gpu_model import build_hip_gan
  intervals, centers, stats = _trainer_set()
  pre = A.DevicePreStep(centers, *stats, mask=(), feats=PV, device=DEV)
  assert pre.PK == P
  B = 4

  def fresh(use_graphs):
    torch.manual_seed(5)
    model = build_hip_gan(2, 2)
    if dtype != 'fp32':
      A.set_compute_dtype(model, dtype)
    store = A.DeviceClipStore(intervals, T=64, hop=3, device=DEV, seed=4, batch_size=B)
    return MixStageTrainStep(model, use_graphs=use_graphs), store

  runs = [fresh(True), fresh(False), fresh(True)]
  forms = [lambda ts, st, k: ts.step_from(st, pre, kind=k), lambda ts, st, k: ts.step_from(st, pre, kind=k),
           lambda ts, st, k: ts.step(*st.draw(pre, B), kind=k)]
  n_graphs = None
  for step, k in enumerate(['G', 'D', 'G', 'D', 'G', 'D']):
    if step in (0, 4):
      for _, st in runs:
        st.new_epoch()
    seen = []
    for (ts, st), form in zip(runs, forms):
      assert form(ts, st, k) == k
      seen.append(([float(l.detach()) for l in ts.losses], ts.state_checksums()))
    assert seen[0] == seen[1], 'step %d: step_from with graphs vs eager' % step
    assert seen[0] == seen[2], 'step %d: step_from vs step() on the twin store\'s draw' % step
    assert np.isfinite(seen[0][0]).all()
    if step == 1:
      n_graphs = len(runs[0][0]._graphs)
      assert n_graphs == 2
    if step > 1:
      assert len(runs[0][0]._graphs) == n_graphs              # no re-capture, new_epoch() included
  # a graph entry holds its store and pre-step: the ids in its key stay theirs while the captured pointers are in use
  assert all(e['feed'].store is runs[0][1] and e['feed'].prestep is pre for e in runs[0][0]._graphs.values())
  cursors = [st.state()['cursor'] for _, st in runs]
  assert cursors == [2 * B] * 3                                # the warm-up passes of the captures gave their draws back
  for ts, st in runs:
    assert st.steps_left == st.W // B - 2
    st.check()
    ts.check_health()




def test_step_from_refuses_a_store_of_another_shard_and_keeps_the_mirror(trainer_globals_restored):
  """A store built as rank 1 of 2 under a single-process trainer is refused before anything is launched; a step that raises leaves
  the host mirror where the device cursor is."""
  import mix_stage_amd as A
  from mix_stage_amd.train_step import MixStageTrainStep
  from test_gpu_model import build_hip_gan
  intervals, centers, stats = _trainer_set()
  pre = A.DevicePreStep(centers, *stats, mask=(), feats=PV, device=DEV)
  torch.manual_seed(5)
  ts = MixStageTrainStep(build_hip_gan(2, 2), use_graphs=True)
  assert ts.shard() == (0, 1)
  other = A.DeviceClipStore(intervals, T=64, hop=3, device=DEV, batch_size=4, rank=1, world=2)
  other.new_epoch()
  with pytest.raises(ValueError, match='rank 1 of 2'):
    ts.step_from(other, pre, kind='G')
  assert other.state()['cursor'] == 0 and other.steps_left == other.W // 8 and len(ts._graphs) == 0
  mine = A.DeviceClipStore(intervals, T=64, hop=3, device=DEV, batch_size=4, trainer=ts)
  assert (mine.rank, mine.world) == (0, 1)
  with pytest.raises(IndexError):
    ts.step_from(mine, pre, kind='G')                         # no epoch started
  mine.new_epoch()
  left = mine.steps_left
  with pytest.raises(ValueError):
    ts.step_from(mine, pre, kind='G', B=mine.max_batch + 1)
  assert mine.steps_left == left and mine.state()['cursor'] == 0
  assert ts.step_from(mine, pre, kind='G') == 'G'
  assert mine.steps_left == left - 1 and mine.state()['cursor'] == 4
  mine.check()


# ---- 6. sampler and metrics glue ---------------------------------------------------------------------------------
def test_interval_feeds_the_sampler():
  from mix_stage_amd import DevicePreStep
  from mix_stage_amd.sample import StyleTransferSampler
  from test_gpu_model import build_hip_gan
  store, pre, intervals, _ = _store_and_pre(LENGTHS, 128, 5, PVS, 64, 7)
  got = store.interval(4, pre)
  assert got[0].shape == (3, 64, 128) and got[1].shape == (3, 64) and got[2].shape == (3, 64, 96) and got[3].shape == (3, 64)
  pose = torch.from_numpy(intervals[4][0][:192]).to(DEV).reshape(3, 64, P)
  audio = torch.from_numpy(intervals[4][1][:192]).to(DEV).reshape(3, 64, 128)
  a, labels, y = pre(pose, audio)
  style = torch.full((3, 64), intervals[4][2], dtype=torch.int64, device=DEV)
  _assert_draw(got, (a, labels, y, style))
  assert store.interval(3, pre)[0].shape == (0, 64, 128)      # 63 frames: no whole window
  # ... and the sampler takes them as they are (full pose: mask = (), the model's P = 104)
  t_intervals, centers, stats = _trainer_set()
  from mix_stage_amd import DeviceClipStore
  t_store = DeviceClipStore(t_intervals, T=64, hop=3, device=DEV)
  t_pre = DevicePreStep(centers, *stats, mask=(), feats=PV, device=DEV)
  windows = t_store.interval(1, t_pre)                          # 90 frames: one window
  assert windows[2].shape == (1, 64, P) and windows[1].dtype == torch.int64 and windows[3].dtype == torch.int64
  sampler = StyleTransferSampler(build_hip_gan(2, 2), num_styles=2, use_graphs=False)
  out = sampler.sample_interval(*windows, all_styles=False)
  name, y_cap, losses = out[0]
  assert y_cap.shape == (1, 64, P) and bool(torch.isfinite(y_cap).all())
