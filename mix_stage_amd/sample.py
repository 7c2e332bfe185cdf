"""Inference / style-transfer driver: the core of the reference's sampling loop, MI355X-native.

Reference: TrainerBase.sample_loop (src/model/trainer.py:740-849) loads one interval, takes ALL of its 64-frame
windows, reshapes them to a single long sequence x:(1, n*64, F), y:(1, n*64, P) (trainer.py:779-786) and runs the
fully-convolutional model once per target style with sample_flag=1, eval-mode BatchNorm and no_grad
(trainer.py:1161-1163); update_kwargs (trainer.py:1367-1386) shifts the style ids modulo the number of styles.

Here the eval forward (running-statistics BatchNorm is folded into each conv kernel's epilogue, MS_BN_EVAL) is captured
into one HIP graph per sequence length and replayed for every target style; inputs live in static HBM buffers.
The pose decoder of such a long sequence (T = n*64, never 64) runs as the wait-free eval form of the chained decoder
(ops.decoder_chain -> ms_decoder_chain_eval_fwd: time tiles of 64 frames, activations resident in LDS through the four
blocks, no workgroup waiting for another one); MS_CHAIN_EVAL=0 keeps it on the blocks one by one.
Dataset I/O, ground-truth loading, metrics and rendering around the loop stay out of scope.

Style mixing (sample_mixed): the generator also takes its style as one float weight per style and frame (EmbLin's 'lin' mode, the
form its training branch uses with argmax=0), which the reference's sampling loop never feeds.  mix_weights() builds such a
(1, T, S) tensor from a mixture of speakers, a per-frame schedule or a ramp between two of them, and sample_mixed() runs the same
long-sequence eval forward on it: one captured graph per sequence length, whose static weight buffer every mixture is copied into.
"""
import numbers

import torch


class StyleTransferSampler:
  def __init__(self, model, num_styles, speaker_names=None, use_graphs=True):
    self.model = model
    self.num_styles = num_styles
    self.speaker = speaker_names or [str(i) for i in range(num_styles)]
    self.use_graphs = use_graphs
    self._graphs = {}
    self._tensors = None

  def _weights_version(self):
    """Sum of the version counters of the model's parameters and buffers: moves when torch changed one of them in place
    (load_weights / load_state_dict, a manual edit)."""
    if self._tensors is None:
      self._tensors = list(self.model.parameters()) + list(self.model.buffers())
    return sum(t._version for t in self._tensors)

  def _replay(self, entry):
    """Replay a captured forward on the weights the model holds NOW.  Under a trainer the kernels read operands derived from the
    weights (16-bit copies, chain weight streams) from buffers that are rebuilt when a weight's version counter moved -- but a
    captured graph holds no such comparison, it reads whatever the buffers held.  The trainer rebuilds them in place behind its
    own updates (a step, ema_weights()); an edit torch made is noticed here, and the buffers of every parameter storage are
    rebuilt in place before the replay, so the graph's pointers stay valid."""
    v = self._weights_version()
    if v != entry['version']:
      from . import ops
      seen = set()
      for p in self.model.parameters():
        if p.is_cuda:
          sp = p.untyped_storage().data_ptr()
          if sp not in seen:
            seen.add(sp)
            ops.refresh_prepared_weights(p)
      entry['version'] = v
    entry['graph'].replay()

  def _kwargs(self, style, T):
    return dict(input_modalities=self.model.input_modalities, desc='test', sample_flag=1, description='test',
                style=style, time_steps=T)

  def style_shifts(self, style, all_styles=True):
    """(style ids, name) pairs of trainer.py:1367-1386 (`sample_all_styles` on/off)."""
    style_id = int(style.reshape(-1)[0].item())
    shifts = range(1, self.num_styles) if all_styles else (1,)
    out = [(style, None)]
    for sh in shifts:
      tgt = (style_id + sh) % self.num_styles
      name = '{}_{}'.format(self.speaker[style_id], self.speaker[tgt]) if all_styles else 'style'
      out.append(((style + sh) % self.num_styles, name))
    return out

  def _forward(self, audio, labels, pose, style):
    T = pose.shape[1]
    with torch.no_grad():
      y_cap, losses, _ = self.model([audio, labels], pose, **self._kwargs(style, T))
    return y_cap, losses

  def sample_interval(self, audio_windows, labels_windows, pose_windows, style_windows, all_styles=True):
    """audio (n,64,F), labels (n,64), pose (n,64,P), style (n,64) of ONE interval, on the GPU.
    Returns [(name, y_cap (1, n*64, P), [losses])] for the speaker's own style and every shifted style."""
    m = self.model
    m.eval()
    n = pose_windows.shape[0]
    audio = audio_windows.reshape(1, -1, audio_windows.shape[-1]).contiguous()
    labels = labels_windows.reshape(1, -1).contiguous()
    pose = pose_windows.reshape(1, -1, pose_windows.shape[-1]).contiguous()
    style0 = style_windows.reshape(1, -1).contiguous()
    results = []
    key = (tuple(audio.shape), tuple(pose.shape))
    entry = self._graphs.get(key) if self.use_graphs else None
    for style, name in self.style_shifts(style0, all_styles):
      if not self.use_graphs:
        y_cap, losses = self._forward(audio, labels, pose, style)
        results.append((name, y_cap, losses))
        continue
      if entry is None:
        entry = self._capture(key, audio, labels, pose, style)
      else:
        torch.rand(1)                       # the forward draws once from the host generator (JL:127)
      st = entry['static']
      for k, src in (('audio', audio), ('labels', labels), ('pose', pose), ('style', style)):
        st[k].copy_(src, non_blocking=True)
      self._replay(entry)
      results.append((name, entry['y_cap'].clone(), [l.clone() for l in entry['losses']]))
    # an in-launch meeting that gave up (the launch did not have the GPU to itself) poisons its outputs with NaN: outside a
    # training step nobody else looks at the error word, so every interval ends with the (synchronising) check -- the caller is
    # about to read the poses anyway.  (The decoder's eval form meets nobody; other kernels of the forward still do.)
    from . import ops16
    ops16.check_meetings()
    return results

  def _mix_rows(self, spec, T):
    """(T, S) float64 rows of one mixture spec (see mix_weights)."""
    S = self.num_styles
    if isinstance(spec, (tuple, list)) and len(spec) > 0 and isinstance(spec[0], str):
      if len(spec) != 3 or spec[0] != 'ramp':
        raise ValueError("a schedule between two mixtures is ('ramp', spec_a, spec_b), got %r" % (spec,))
      a, b = self._mix_rows(spec[1], T), self._mix_rows(spec[2], T)
      b = b.to(a.device)
      # a_t = t / (T - 1), 0 for a single frame: the first frame is spec_a, the last one spec_b
      at = (torch.arange(T, dtype=torch.float64, device=a.device) / max(T - 1, 1)).unsqueeze(1)
      return (1.0 - at) * a + at * b
    if isinstance(spec, dict):
      row = torch.zeros(S, dtype=torch.float64)
      for k, v in spec.items():
        if isinstance(k, str):
          if k not in self.speaker:
            raise ValueError('unknown speaker %r (known: %s)' % (k, ', '.join(map(str, self.speaker))))
          k = self.speaker.index(k)
        elif not isinstance(k, numbers.Integral) or isinstance(k, bool) or not 0 <= k < S:
          raise ValueError('style id %r is not one of 0..%d' % (k, S - 1))
        row[int(k)] += float(v)
      rows = row
    else:
      try:
        rows = spec.to(torch.float64) if isinstance(spec, torch.Tensor) else torch.as_tensor(spec, dtype=torch.float64)
      except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError('a mixture is a dict, a length-%d vector, a (T, %d) or (n, 64, %d) schedule or a ramp: %s' % (S, S, S, e))
    if rows.dim() == 1 and rows.shape[0] == S:
      rows = rows.unsqueeze(0).expand(T, S)
    elif rows.dim() == 3 and rows.shape[-1] == S and rows.shape[0] * rows.shape[1] == T:
      rows = rows.reshape(T, S)                       # windows of one interval, concatenated like the inputs
    elif not (rows.dim() == 2 and rows.shape == (T, S)):
      raise ValueError('style weights of shape %s fit neither (%d,), (%d, %d) nor (n, 64, %d) with n * 64 = %d'
                       % (tuple(rows.shape), S, T, S, S, T))
    if not bool(torch.isfinite(rows).all()):
      raise ValueError('style weights must be finite')
    return rows

  def mix_weights(self, spec, T):
    """float32 (1, T, S) style weights for T frames.  `spec` is
      * a dict {style id or speaker name: weight} (styles not named weigh 0),
      * a length-S sequence or tensor: the same weights on every frame,
      * a (T, S) or (n, 64, S) tensor: one row per frame,
      * ('ramp', spec_a, spec_b): (1 - a_t) * A + a_t * B per frame with a_t = t / (T - 1) (a_t = 0 for T == 1).
    Weights are used as given -- nothing is normalised, the generator takes any finite float.  Computed in float64, then cast.
    Pure torch: a tensor spec stays on its device, everything else is built on the CPU."""
    if not isinstance(T, numbers.Integral) or T < 1:
      raise ValueError('T = %r frames' % (T,))
    return self._mix_rows(spec, int(T)).to(torch.float32).reshape(1, int(T), self.num_styles).contiguous()

  def sample_mixed(self, audio_windows, labels_windows, pose_windows, mixes):
    """audio (n,64,F), labels (n,64), pose (n,64,P) of ONE interval, on the GPU; mixes: [(name, spec)], spec as in mix_weights.
    Returns [(name, y_cap (1, n*64, P), [losses])], one entry per mixture.  With graphs, ONE capture per sequence length serves
    every mixture, schedule and ramp: its style input is a static (1, n*64, S) weight buffer."""
    m = self.model
    m.eval()
    audio = audio_windows.reshape(1, -1, audio_windows.shape[-1]).contiguous()
    labels = labels_windows.reshape(1, -1).contiguous()
    pose = pose_windows.reshape(1, -1, pose_windows.shape[-1]).contiguous()
    T = pose.shape[1]
    results = []
    key = ('mix', tuple(audio.shape), tuple(pose.shape))         # apart from the id form's graph of the same lengths
    entry = self._graphs.get(key) if self.use_graphs else None
    for name, spec in mixes:
      style = self.mix_weights(spec, T).to(pose.device)
      if not self.use_graphs:
        y_cap, losses = self._forward(audio, labels, pose, style)
        results.append((name, y_cap, losses))
        continue
      if entry is None:
        entry = self._capture(key, audio, labels, pose, style)
      else:
        torch.rand(1)                       # the forward draws once from the host generator (JL:127)
      st = entry['static']
      for k, src in (('audio', audio), ('labels', labels), ('pose', pose), ('style', style)):
        st[k].copy_(src, non_blocking=True)
      self._replay(entry)
      results.append((name, entry['y_cap'].clone(), [l.clone() for l in entry['losses']]))
    from . import ops16
    ops16.check_meetings()                  # as sample_interval: a meeting that gave up poisons its outputs, nobody else looks
    return results

  def _capture(self, key, audio, labels, pose, style):
    st = dict(audio=audio.clone(), labels=labels.clone(), pose=pose.clone(), style=style.clone())
    rng = torch.get_rng_state()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      self._forward(st['audio'], st['labels'], st['pose'], st['style'])    # sizes the workspace
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    torch.set_rng_state(rng)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
      y_cap, losses = self._forward(st['audio'], st['labels'], st['pose'], st['style'])
    entry = dict(graph=g, static=st, y_cap=y_cap, losses=[l for l in losses], version=self._weights_version())
    self._graphs[key] = entry
    return entry
