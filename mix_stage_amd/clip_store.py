"""Device-resident clip store: the batch itself, drawn on the MI355X inside the (captured) training step.

Reference: the training loop reads its batches through a DataLoader with num_workers=0 over per-interval HDF5 files
(src/model/trainer.py:603); a captured step here runs in 0.75 to 4.4 ms, i.e. consumes 10 000 to 20 000 clips a
second.  A whole PATS speaker set fits in HBM many times over (30 h of one speaker at 15 fps = 1.6 M frames x (104 + 128) fp32 = 1.5 GB),
so the raw frames of every interval are kept on the device, concatenated frame by frame, and one launch (ms_clip_draw) picks the step's
B windows from a device-side epoch order, gathers them, runs the pre-step on them -- bit for bit what DevicePreStep.__call__ gives on the
gathered clips -- and writes the result where the step reads it.  A one-thread launch (ms_clip_advance) then moves the cursor, so a
replayed graph walks through an epoch with no host work but the replay.

Host side (pure functions, no GPU needed): window_table, epoch_order, steps_per_epoch, draw_positions.
"""
import ctypes

import torch

from ._lib import check, lib

_vp = ctypes.c_void_p
_INT32_MIN, _INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _p(t):
  return None if t is None else _vp(t.data_ptr())


def window_table(lengths, T, hop):
  """-> (win_interval, win_start), int64 tensors: the windows of interval i start at 0, hop, 2*hop, ... while start + T <= lengths[i]."""
  T, hop = int(T), int(hop)
  if T < 1:
    raise ValueError('window_table: T = %d' % T)
  if hop < 1:
    raise ValueError('window_table: hop = %d, must be >= 1' % hop)
  win_interval, win_start = [], []
  for i, n in enumerate(lengths):
    n = int(n)
    if n >= T:
      starts = range(0, n - T + 1, hop)
      win_interval.extend([i] * len(starts))
      win_start.extend(starts)
  return torch.tensor(win_interval, dtype=torch.int64), torch.tensor(win_start, dtype=torch.int64)


def epoch_order(W, seed, epoch):
  """The order an epoch draws the W windows in: the same on every rank of a job (same seed), another one every epoch."""
  return torch.randperm(int(W), generator=torch.Generator().manual_seed(int(seed) + int(epoch))).to(torch.int32)


def steps_per_epoch(n_order, B, world=1):
  """Whole steps in an order of n_order windows: every step takes world * B of them; the remainder is not drawn."""
  return int(n_order) // (int(B) * int(world))


def draw_positions(cursor, B, rank=0, world=1):
  """The positions of the order that rank `rank` draws in the step that starts at `cursor` (the kernel's arithmetic): clip b is
  window order[cursor + rank * B + b]; the step moves the cursor by world * B."""
  if not 0 <= rank < world:
    raise ValueError('rank %d of world %d' % (rank, world))
  return range(cursor + rank * B, cursor + rank * B + B)


def _check_intervals(shapes, styles, T, hop):
  """The constructor's checks, on shapes alone (before any device use).  shapes: [(T_i, P, T_i', F)]."""
  if int(hop) < 1:
    raise ValueError('DeviceClipStore: hop = %d, must be >= 1' % hop)
  if int(T) < 1:
    raise ValueError('DeviceClipStore: T = %d' % T)
  if not shapes:
    raise ValueError('DeviceClipStore: no interval, so no window at all')
  P, F = shapes[0][1], shapes[0][3]
  for i, (n, p, na, f) in enumerate(shapes):
    if p != P or f != F:
      raise ValueError('DeviceClipStore: interval %d has P = %d, F = %d; interval 0 has %d, %d' % (i, p, f, P, F))
    if n != na:
      raise ValueError('DeviceClipStore: interval %d has %d pose frames and %d audio frames' % (i, n, na))
  for i, s in enumerate(styles):
    if int(s) != s or not _INT32_MIN <= int(s) <= _INT32_MAX:
      raise ValueError('DeviceClipStore: style id %r of interval %d is outside int32' % (s, i))
  lengths = [s[0] for s in shapes]
  if not any(n >= T for n in lengths):
    raise ValueError('DeviceClipStore: no interval holds a window of T = %d frames (longest: %d): no window at all' % (T, max(lengths)))
  return lengths, P, F


class DeviceClipStore:
  """The raw frames of a speaker set on the device, and the epoch's draw state next to them.

  intervals: list of (pose (T_i, P), audio (T_i, F), style_id), fp32 tensors on the CPU or the device; from_rows() takes rows that are
  already concatenated on the device (large sets are assembled chunk by chunk by the caller).  Windows of T frames start every `hop`
  frames inside an interval (window_table; hop defaults to T).  rank / world: this process draws its own B of every world * B windows
  of the order.  Both are fixed at construction: given explicitly, or the trainer's (trainer=ts: MixStageTrainStep.shard()), or 0 / 1;
  step_from() refuses a store whose rank / world are not its trainer's.  batch_size: the B that steps_left and
  MixStageTrainStep.step_from count with (default: the B of the last draw); max_batch: the largest B ever drawn -- the order buffer
  is allocated once with W + max_batch * world slots and padded with -1, so a draw at the end of the order reads inside it whatever
  the cursor holds, and new_epoch() never reallocates under a captured graph.
  Raises ValueError for: no window at all, hop < 1, ragged P / F, a style id outside int32."""

  def __init__(self, intervals, T=64, hop=None, device='cuda:0', rank=None, world=None, seed=0, batch_size=None, max_batch=256,
               trainer=None):
    intervals = list(intervals)
    hop = T if hop is None else hop
    shapes = []
    for i, (pose, audio, _) in enumerate(intervals):
      if pose.dim() != 2 or audio.dim() != 2 or pose.dtype != torch.float32 or audio.dtype != torch.float32:
        raise ValueError('DeviceClipStore: interval %d: pose (T_i, P) and audio (T_i, F) must be 2-D float32 tensors' % i)
      shapes.append((pose.shape[0], pose.shape[1], audio.shape[0], audio.shape[1]))
    styles = [it[2] for it in intervals]
    lengths, P, F = _check_intervals(shapes, styles, T, hop)
    dev = torch.device(device)
    pose_rows = torch.cat([it[0].to(dev) for it in intervals]).contiguous()
    audio_rows = torch.cat([it[1].to(dev) for it in intervals]).contiguous()
    self._setup(pose_rows, audio_rows, lengths, styles, T, hop, rank, world, seed, batch_size, max_batch, trainer)

  @classmethod
  def from_rows(cls, pose_rows, audio_rows, lengths, styles, T=64, hop=None, rank=None, world=None, seed=0, batch_size=None,
                max_batch=256, trainer=None):
    """pose_rows (R, P), audio_rows (R, F): contiguous fp32 device tensors, the intervals one after the other; lengths / styles: the
    frames and the style id of each.  The rows are used in place (no copy): they may be larger than 2 GiB each."""
    hop = T if hop is None else hop
    lengths, styles = [int(n) for n in lengths], list(styles)
    if pose_rows.dim() != 2 or audio_rows.dim() != 2 or pose_rows.dtype != torch.float32 or audio_rows.dtype != torch.float32:
      raise ValueError('DeviceClipStore.from_rows: pose_rows (R, P) and audio_rows (R, F) must be 2-D float32 tensors')
    if len(lengths) != len(styles):
      raise ValueError('DeviceClipStore.from_rows: %d lengths, %d styles' % (len(lengths), len(styles)))
    if sum(lengths) != pose_rows.shape[0] or pose_rows.shape[0] != audio_rows.shape[0]:
      raise ValueError('DeviceClipStore.from_rows: the lengths sum to %d rows, pose_rows has %d, audio_rows %d'
                       % (sum(lengths), pose_rows.shape[0], audio_rows.shape[0]))
    _check_intervals([(n, pose_rows.shape[1], n, audio_rows.shape[1]) for n in lengths], styles, T, hop)
    if not (pose_rows.is_cuda and audio_rows.is_cuda and pose_rows.is_contiguous() and audio_rows.is_contiguous()):
      raise ValueError('DeviceClipStore.from_rows: the rows must be contiguous tensors on the device')
    self = cls.__new__(cls)
    self._setup(pose_rows, audio_rows, lengths, styles, T, hop, rank, world, seed, batch_size, max_batch, trainer)
    return self

  def _setup(self, pose_rows, audio_rows, lengths, styles, T, hop, rank, world, seed, batch_size, max_batch, trainer):
    dev = pose_rows.device
    self.dev, self.T, self.hop, self.seed = dev, int(T), int(hop), int(seed)
    self.pose_rows, self.audio_rows = pose_rows, audio_rows
    self.R, self.P, self.F = pose_rows.shape[0], pose_rows.shape[1], audio_rows.shape[1]
    self.lengths, self.styles = [int(n) for n in lengths], [int(s) for s in styles]
    starts = [0]
    for n in self.lengths:
      starts.append(starts[-1] + n)
    self.row_start = starts[:-1]
    self.win_interval, self.win_start = window_table(self.lengths, self.T, self.hop)
    self.W = int(self.win_interval.numel())
    win_row = torch.tensor(self.row_start, dtype=torch.int64)[self.win_interval] + self.win_start
    self._win_row = win_row.to(dev)
    self._win_style = torch.tensor(self.styles, dtype=torch.int32)[self.win_interval].to(dev)
    if (rank is None) != (world is None):
      raise ValueError('DeviceClipStore: rank and world come together')
    if world is None:
      rank, world = trainer.shard() if trainer is not None else (0, 1)
    if not 0 <= rank < world:
      raise ValueError('DeviceClipStore: rank %d of world %d' % (rank, world))
    self.rank, self.world = int(rank), int(world)
    self.batch_size = None if batch_size is None else int(batch_size)
    self.max_batch = max(int(max_batch), self.batch_size or 0)
    self._state = torch.zeros(4, dtype=torch.int32, device=dev)       # error flag | cursor | 0 | 0
    self._indices = torch.full((self.max_batch,), -1, dtype=torch.int32, device=dev)
    self._last_B = 0
    self._order = None          # (W + max_batch * world) int32, -1 behind the epoch's order: allocated by the first new_epoch()
    self.n_order = 0
    self.epoch = -1
    self._cursor = 0            # host mirror of state word 1

  # ---- the epoch --------------------------------------------------------------------------------------------
  def new_epoch(self, order=None):
    """Start an epoch: write its order, zero the cursor and the error flag, on the current stream.  ORDERING RULE (that of
    MixStageTrainStep.epoch_end): call it between two steps, from the thread and under the stream that steps; stream order does
    the rest.  order=None: epoch_order(W, seed, epoch), epoch counting from 0.  A caller's int sequence or tensor of window ids
    (at most W of them) is taken as given -- the place for a class-alternating sampler.  Captured steps need no re-capture."""
    if self.dev.type == 'cuda' and torch.cuda.is_current_stream_capturing():
      raise RuntimeError('DeviceClipStore.new_epoch inside a stream capture')
    self.epoch += 1
    if order is None:
      order = epoch_order(self.W, self.seed, self.epoch)
    else:
      order = torch.as_tensor(order)
      if order.dim() != 1 or order.dtype.is_floating_point or order.dtype == torch.bool:
        raise ValueError('DeviceClipStore.new_epoch: order must be a 1-D sequence of window ids')
      if order.numel() > self.W:
        raise ValueError('DeviceClipStore.new_epoch: %d entries, the store has %d windows (no drawing with replacement)'
                         % (order.numel(), self.W))
      order = order.to(torch.int32)
    if self._order is None:
      self._order = torch.full((self.W + self.max_batch * self.world,), -1, dtype=torch.int32, device=self.dev)
    n = int(order.numel())
    self._order[:n].copy_(order)
    self._order[n:].fill_(-1)
    self._state.zero_()
    self.n_order, self._cursor = n, 0

  @property
  def steps_left(self):
    """Whole steps of batch_size left in this epoch's order, by the host mirror of the cursor."""
    if self.batch_size is None:
      raise ValueError('DeviceClipStore.steps_left: no batch_size given and nothing drawn yet')
    return steps_per_epoch(self.n_order - self._cursor, self.batch_size, self.world)

  def _room(self, B):
    """The host's look before a draw: IndexError past the end of the order, before anything is launched."""
    if self._order is None:
      raise IndexError('DeviceClipStore: no epoch started: call new_epoch()')
    if not 1 <= B <= self.max_batch:
      raise ValueError('DeviceClipStore: B = %d, the store was built for at most max_batch = %d' % (B, self.max_batch))
    if self._cursor + self.world * B > self.n_order:
      raise IndexError('DeviceClipStore: the order of %d windows is drawn up to %d, a step takes %d: call new_epoch()'
                       % (self.n_order, self._cursor, self.world * B))

  def _issued(self, B):
    """A draw of B has been launched (or a graph that holds one replayed): the host mirror follows the device cursor."""
    self._cursor += self.world * B
    self.batch_size = self.batch_size or B

  # ---- drawing ----------------------------------------------------------------------------------------------
  def _check_prestep(self, prestep):
    if prestep.P != self.P or prestep.audio_mean.numel() != self.F or prestep.dev != self.dev:
      raise ValueError('DeviceClipStore: the pre-step is for P = %d, F = %d on %s; the store holds P = %d, F = %d on %s'
                       % (prestep.P, prestep.audio_mean.numel(), prestep.dev, self.P, self.F, self.dev))

  def _launch(self, prestep, audio, labels, y, style, full):
    """The two launches of a draw into (B,T,.) buffers, on the current stream: no allocation, no synchronisation, no host state."""
    B = audio.shape[0]
    s = _vp(torch.cuda.current_stream().cuda_stream)
    ps = prestep
    check(lib().ms_clip_draw(_p(self.pose_rows), _p(self.audio_rows), self.R, _p(self._win_row), _p(self._win_style), self.W,
                             _p(self._order), self._order.numel(), _p(self._state), B, self.T, self.rank, self.world, _p(ps.keep),
                             _p(ps.centers), ps.M, ps.feats, _p(ps.pose_mean), _p(ps.pose_inv), _p(ps.audio_mean), _p(ps.audio_inv),
                             self.P, ps.PK, self.F, _p(audio), _p(labels), _p(y), _p(style), _p(full), _p(self._indices), s),
          'ms_clip_draw')
    check(lib().ms_clip_advance(_p(self._state), self.world * B, s), 'ms_clip_advance')
    self._last_B = B

  def _check_buffers(self, prestep, audio, labels, y, style, full):
    B = audio.shape[0]
    want = [('audio', audio, (B, self.T, self.F), torch.float32), ('labels', labels, (B, self.T), torch.int64),
            ('y', y, (B, self.T, prestep.PK), torch.float32), ('style', style, (B, self.T), torch.int64)]
    if full is not None:
      want.append(('full', full, (B, self.T, self.P), torch.float32))
    for name, t, shape, dtype in want:
      if tuple(t.shape) != shape or t.dtype != dtype or t.device != self.dev or not t.is_contiguous():
        raise ValueError('DeviceClipStore.draw_into: %s must be a contiguous %s tensor of shape %s on %s' % (name, dtype, shape, self.dev))

  def draw_into(self, prestep, audio, labels, y, style, full=None, _unchecked=False):
    """Draw the next B = audio.shape[0] windows into the caller's buffers: audio (B,T,F) fp32 z-normed, labels (B,T) int64,
    y (B,T,PK) fp32 z-normed kept columns, style (B,T) int64, full (B,T,P) fp32 z-normed full pose (the gt_full_norm of the
    metrics) or None.  Raises IndexError past the end of the order before anything is launched.  Inside a stream capture the host
    mirror of the cursor stays (nothing runs): move it with mark_drawn() for the replays."""
    self._check_prestep(prestep)
    self._check_buffers(prestep, audio, labels, y, style, full)
    B = audio.shape[0]
    capturing = torch.cuda.is_current_stream_capturing()
    if _unchecked or capturing:          # (_unchecked: tests of the device guard, no look at the end of the order)
      if self._order is None or not 1 <= B <= self.max_batch:
        raise ValueError('DeviceClipStore: B = %d (at most max_batch = %d), epoch started: %s' % (B, self.max_batch, self._order is not None))
    else:
      self._room(B)
    self._launch(prestep, audio, labels, y, style, full)
    if not capturing:
      self._issued(B)

  def draw(self, prestep, B, full_pose=False, _unchecked=False):
    """-> (audio, labels, y, style[, pose_full_norm]) of the next B windows, as MixStageTrainStep.step takes them."""
    dev = self.dev
    out = [torch.empty((B, self.T, self.F), dtype=torch.float32, device=dev), torch.empty((B, self.T), dtype=torch.int64, device=dev),
           torch.empty((B, self.T, prestep.PK), dtype=torch.float32, device=dev), torch.empty((B, self.T), dtype=torch.int64, device=dev)]
    if full_pose:
      out.append(torch.empty((B, self.T, self.P), dtype=torch.float32, device=dev))
    self.draw_into(prestep, *out, _unchecked=_unchecked)
    return tuple(out)

  def mark_drawn(self, B, steps=1):
    """Move the host mirror for `steps` replays of a captured draw of B (IndexError past the end, as a draw)."""
    for _ in range(steps):
      self._room(B)
      self._issued(B)

  @property
  def last_indices(self):
    """(B) int32 on the device: the window ids of the last draw (-1: no window)."""
    return self._indices[:self._last_B]

  # ---- state --------------------------------------------------------------------------------------------------
  def check(self):
    """Reads state word 0 (synchronises) and raises if a draw met "no window": a position past the order or an id outside [0, W)."""
    if int(self._state[0]) != 0:
      raise RuntimeError('DeviceClipStore: a draw ran past the epoch\'s order or met a window id outside [0, %d): those clips were '
                         'written as zeros with index -1.  new_epoch() clears the flag' % self.W)

  def state(self):
    """dict(seed, epoch, cursor, order) for a resumable checkpoint (next to ts.optimizer_state()).  Synchronises."""
    order = self._order[:self.n_order].cpu() if self._order is not None else torch.zeros(0, dtype=torch.int32)
    return dict(seed=self.seed, epoch=self.epoch, cursor=int(self._state[1]), order=order)

  def set_state(self, d):
    """Write back what state() returned.  Between steps, as new_epoch()."""
    self.seed = int(d['seed'])
    self.epoch = int(d['epoch']) - 1
    self.new_epoch(d['order'])
    cursor = int(d['cursor'])
    self._state[1:2].fill_(cursor)
    self._cursor = cursor

  # ---- inference ----------------------------------------------------------------------------------------------
  def interval(self, i, prestep):
    """The non-overlapping windows of interval i, through the same kernel: (audio (n,T,F), labels (n,T), y (n,T,PK), style (n,T)) --
    the form StyleTransferSampler.sample_interval takes.  Frames past the last whole window are left out.  Does not move the epoch."""
    self._check_prestep(prestep)
    n, T, dev = self.lengths[i] // self.T, self.T, self.dev
    audio = torch.empty((n, T, self.F), dtype=torch.float32, device=dev)
    labels = torch.empty((n, T), dtype=torch.int64, device=dev)
    y = torch.empty((n, T, prestep.PK), dtype=torch.float32, device=dev)
    style = torch.empty((n, T), dtype=torch.int64, device=dev)
    if n == 0:
      return audio, labels, y, style
    win_row = self.row_start[i] + T * torch.arange(n, dtype=torch.int64, device=dev)
    win_style = torch.full((n,), self.styles[i], dtype=torch.int32, device=dev)
    order = torch.arange(n, dtype=torch.int32, device=dev)
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    indices = torch.empty(n, dtype=torch.int32, device=dev)
    ps = prestep
    check(lib().ms_clip_draw(_p(self.pose_rows), _p(self.audio_rows), self.R, _p(win_row), _p(win_style), n, _p(order), n, _p(state),
                             n, T, 0, 1, _p(ps.keep), _p(ps.centers), ps.M, ps.feats, _p(ps.pose_mean), _p(ps.pose_inv),
                             _p(ps.audio_mean), _p(ps.audio_inv), self.P, ps.PK, self.F, _p(audio), _p(labels), _p(y), _p(style), None,
                             _p(indices), _vp(torch.cuda.current_stream().cuda_stream)), 'ms_clip_draw')
    return audio, labels, y, style


class StoreFeed:
  """What MixStageTrainStep.step_from hands to the shared step code in place of four input tensors: where the batch comes from."""

  def __init__(self, store, prestep, B):
    store._check_prestep(prestep)
    self.store, self.prestep, self.B = store, prestep, int(B)
    self.shapes = ((self.B, store.T, store.F), (self.B, store.T, prestep.PK))
    # (ids: the graph entry made under this key holds the store and the pre-step -- MixStageTrainStep._capture -- so while the entry
    # lives neither id can be handed to another object)
    self.key = ('store', id(store), id(prestep), self.B)

  def alloc(self):
    """The static input buffers of a captured step."""
    return {n: torch.zeros(shape, dtype=dtype, device=self.store.dev) for n, (shape, dtype) in self.alloc_spec().items()}

  def fits(self, st):
    """Do the static buffers of an earlier step() have the draw's shapes and dtypes?"""
    want = self.alloc_spec()
    return all(tuple(st[n].shape) == shape and st[n].dtype == dtype and st[n].is_contiguous() for n, (shape, dtype) in want.items())

  def alloc_spec(self):
    bt = (self.B, self.store.T)
    return dict(audio=(self.shapes[0], torch.float32), labels=(bt, torch.int64), pose=(self.shapes[1], torch.float32),
                style=(bt, torch.int64))

  def draw(self):
    """Eager mode: the draw into fresh tensors; the host mirror follows."""
    st = {n: torch.empty(shape, dtype=dtype, device=self.store.dev) for n, (shape, dtype) in self.alloc_spec().items()}
    self.launch(st)
    self.issued()
    return st['audio'], st['labels'], st['pose'], st['style']

  def issued(self):
    """The step's draw has been launched or replayed: the host mirror moves, once per step."""
    self.store._issued(self.B)

  def launch(self, st):
    """The head of the step: draw into the static buffers (two launches; captured with the step)."""
    self.store._launch(self.prestep, st['audio'], st['labels'], st['pose'], st['style'], None)

  def save(self):
    return self.store._state.clone()

  def restore(self, saved):
    self.store._state.copy_(saved)
