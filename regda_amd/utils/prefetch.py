"""Host -> device input staging for the training loops.

The reference moves every tensor of a batch with `.cuda()` inside the iteration (tools/train_ssl_reg.py:200-206:
images_s, label_s, images_t, label_t_soft, regs_t), a synchronous pageable copy of ~84 MB per 8 + 8 batch of 512 x 512
tiles with int64 labels / region maps.  Here the loader's batches sit in PINNED host memory and are copied by a
dedicated HIP stream into one of `depth` device-resident slots while the previous step computes; the consumer only
waits for an event.  The tensors keep the reference's dtypes and shapes (the int64 API is the boundary).

With `augment`, the host batches are RAW tiles (uint8 HWC images, uint8 labels, f32 soft labels, int32 region maps): they
are copied into device staging buffers on the copy stream and the training augmentation (regda_amd.aug) writes the
step's tensors from them on the same stream, one launch per domain, with each sample's parameters drawn on the host
when the batch is staged, in batch order.

With `regions` as well, a domain whose roles name a 'mask_sup' tensor that the host batches do not carry gets its region
map from the raw uint8 tile itself (regda_amd.gast.superpixels.SuperPixelsSLIC, rgda_superpixels) on the copy stream; the
map is the augmentation's `regs` input, so it goes through the same crop and dihedral element as the image.

With `mix`, one more launch on the copy stream (rgda_domain_mix) pastes part of the source slot over the target slot
after everything else has been written there: cross-domain ClassMix / CutMix, drawn per batch on the host when the batch
is staged (regda_amd.aug.mix.DomainMix)."""
import torch

from .. import ops


class DevicePrefetcher:
    def __init__(self, host_batches, device=None, depth=2, into=None, augment=None, regions=None, mix=None):
        """host_batches: list of {name: CPU tensor or None} with identical shapes; cycled through in order.
        into: {name: device tensor} -- stage every batch straight into THESE tensors (one slot: the static input
        buffers of a recorded step, SSLStep.static_inputs()); `release()` must then be given the event after which the
        step no longer reads its inputs (SSLStep.inputs_consumed).
        augment: list of (pipeline, roles), one per domain: a regda_amd.aug pipeline and {role: name} with the roles
        'image' (uint8 [N][H][W][3]), 'mask' (uint8 [N][H][W] class labels), 'soft' (f32 [N][C][H][W]) and 'mask_sup'
        (int32 [N][H][W] region ids); the named host tensors are raw and their slot tensors hold the pipeline's outputs
        (f32 [N][3][Ho][Wo], int64 [N][Ho][Wo], f32 [N][C][Ho][Wo], int64 [N][1][Ho][Wo]).  Names in no role are
        copied as they are.
        regions: a SuperPixelsSLIC (needs `augment`).  Where a domain's roles name 'mask_sup' and the host batches have
        no tensor of that name (absent or None), the int32 region map is generated from the staged raw image and
        delivered under that name as the pipeline's int64 [N][1][Ho][Wo] output.  A batch that carries its 'mask_sup' is
        staged as without `regions`.
        mix: (domain_mix, roles_s, roles_t) -- a regda_amd.aug.mix.DomainMix and the {role: name} of the source
        ('image', 'mask') and target ('image' and any of 'mask', 'soft', 'mask_sup') slot tensors (f32 [N][3][H][W],
        int64 [N][H][W], f32 [N][C][H][W], int64 [N][1][H][W]: the augmentation's outputs, or what the host batches
        carry; the int64 maps with or without the unit axis).  The target tensors of a slot are rewritten in place where the batch's draw pastes; a pasted pixel gets
        the source image and label, a one-hot soft label and region 0.  `mix_flag` (device int32) is set to 1 by a source
        label that is neither a class nor the ignore label."""
        if regions is not None and not augment:
            raise ValueError('DevicePrefetcher: regions= generates the region maps from the RAW uint8 tiles, which only '
                             'the augment= path stages; give augment=[(pipeline, roles), ...] as well')
        assert host_batches and (into is not None or depth >= 2)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.host = [{k: (None if v is None else v.contiguous().pin_memory()) for k, v in b.items()} for b in host_batches]
        self.augment = []
        shapes = {k: (None if v is None else (tuple(v.shape), v.dtype)) for k, v in self.host[0].items()}
        for pipe, roles in (augment or ()):
            gen = roles.get('mask_sup') if regions is not None and self.host[0].get(roles.get('mask_sup')) is None else None
            roles = {r: k for r, k in roles.items() if self.host[0].get(k) is not None}
            img = self.host[0][roles['image']]
            n, h, w, _ = img.shape
            ho, wo = pipe.out_size(h, w)
            out = dict(image=((n, 3, ho, wo), torch.float32), mask=((n, ho, wo), torch.int64),
                       mask_sup=((n, 1, ho, wo), torch.int64))
            if 'soft' in roles:
                out['soft'] = ((n, self.host[0][roles['soft']].shape[1], ho, wo), torch.float32)
            for r, k in roles.items():
                shapes[k] = out[r]
            # device staging of the raw batch (one set: written and read in copy-stream order), the device tables and
            # the per-batch parameter table
            raw = {r: torch.empty_like(self.host[0][k], device=self.device) for r, k in roles.items()}
            if gen is not None:
                # generated on the device: no host tensor, but a slot tensor like any other mask_sup
                shapes[gen] = out['mask_sup']
                raw['mask_sup'] = torch.empty((n, h, w), dtype=torch.int32, device=self.device)
                raw['sup_count'] = torch.empty((n,), dtype=torch.int32, device=self.device)
                regions.reserve(n, h, w, self.device)
            tables = pipe.device_tables(self.device)
            prm = torch.empty(n, pipe.param_cols, dtype=torch.int32, device=self.device)
            self.augment.append((pipe, roles, raw, tables, prm, gen))
        if into is not None:
            depth = 1
            self.slots = [{k: into.get(k) for k in shapes}]
            for k, v in shapes.items():
                t = self.slots[0][k]
                assert (v is None) == (t is None) and (v is None or (tuple(t.shape) == v[0] and t.dtype == v[1])), k
        else:
            self.slots = [{k: (None if v is None else torch.empty(v[0], dtype=v[1], device=self.device))
                           for k, v in shapes.items()} for _ in range(depth)]
        self.regions = regions
        self.mix = None
        if mix is not None:
            dmix, roles_s, roles_t = mix
            if 'image' not in roles_s or 'mask' not in roles_s or 'image' not in roles_t:
                raise ValueError("DevicePrefetcher: mix= needs the source's 'image' and 'mask' and the target's 'image'")
            if 'mask' not in roles_t and 'soft' not in roles_t:
                raise ValueError("DevicePrefetcher: mix= needs a target 'mask' or 'soft' role: without either the "
                                 'target has no supervision to mix (the online-teacher batch labels it inside the step)')
            unknown = (set(roles_s) - {'image', 'mask'}) | (set(roles_t) - {'image', 'mask', 'soft', 'mask_sup'})
            missing = [k for k in list(roles_s.values()) + list(roles_t.values()) if shapes.get(k) is None]
            if unknown or missing:
                raise ValueError('DevicePrefetcher: mix= roles %s unknown, tensors %s not in the batches'
                                 % (sorted(unknown), missing))
            (n, _, h, w), c = shapes[roles_t['image']][0], dmix.class_num
            maps = [((n, h, w), torch.int64), ((n, 1, h, w), torch.int64)]
            want = {'image': [((n, 3, h, w), torch.float32)], 'mask': maps, 'soft': [((n, c, h, w), torch.float32)],
                    'mask_sup': maps}
            for roles in (roles_s, roles_t):
                for r, k in roles.items():
                    if shapes[k] not in want[r]:
                        raise ValueError('DevicePrefetcher: mix= pairs the source and target slots pixel by pixel at %d '
                                         'classes: %r (%s) must be %s, got %s' % (c, k, r, want[r], shapes[k]))
            self.mix = (dmix, dict(roles_s), dict(roles_t), (h, w))
            self.mix_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.single = into is not None
        self.copy_stream = torch.cuda.Stream(device=self.device)
        if self.augment or self.mix:
            self.copy_stream.wait_stream(torch.cuda.current_stream())     # the staging buffers and tables made above
        self.copied = [None] * depth        # event: the slot holds its batch
        self.consumed = [None] * depth      # event: the step that read the slot has been enqueued and finished with it
        self.i = 0                          # index of the next batch handed out
        self.bytes_per_batch = sum(v.numel() * v.element_size() for v in self.host[0].values() if v is not None)
        if self.single:
            # `into` are the live input buffers of a recorded step: whatever has been enqueued on the current stream so
            # far (a step still reading them) must be done before the first batch lands there
            self.consumed[0] = torch.cuda.current_stream().record_event()
        self._stage(0)

    def _stage(self, i):
        slot = i % len(self.slots)
        src = self.host[i % len(self.host)]
        if self.augment:
            self._stage_augmented(slot, src)
            return
        if self.consumed[slot] is not None:
            self.copy_stream.wait_event(self.consumed[slot])
        with torch.cuda.stream(self.copy_stream):
            for k, dst in self.slots[slot].items():
                if dst is not None:
                    dst.copy_(src[k], non_blocking=True)
            self._mix(slot)
            self.copied[slot] = self.copy_stream.record_event()

    def _stage_augmented(self, slot, src):
        # the raw bytes and the drawn parameters go to the staging buffers first (nothing the step reads); only the
        # writes into the slot wait for the step that reads it
        with ops.use_stream(self.copy_stream):
            done = set()
            for pipe, roles, raw, _, prm, gen in self.augment:
                for r, k in roles.items():
                    raw[r].copy_(src[k], non_blocking=True)
                    done.add(k)
                if gen is not None:
                    self.regions(raw['image'], out=(raw['mask_sup'], raw['sup_count']))
                    done.add(gen)
                n, h, w, _ = raw['image'].shape
                p = pipe.params(n, h, w)
                pipe.check_params(p, h, w)
                prm.copy_(p.pin_memory(), non_blocking=True)
            if self.consumed[slot] is not None:
                self.copy_stream.wait_event(self.consumed[slot])
            dst = self.slots[slot]
            for k, t in dst.items():
                if t is not None and k not in done:
                    t.copy_(src[k], non_blocking=True)
            for pipe, roles, raw, (lut, llut), prm, gen in self.augment:
                out = {'image': dst[roles['image']], 'label': dst.get(roles.get('mask')), 'soft': dst.get(roles.get('soft')),
                       'regs': dst.get(roles.get('mask_sup', gen))}
                pipe.launch(raw['image'], prm, lut, tuple(out['image'].shape[2:]), label=raw.get('mask'),
                            label_lut=llut, soft=raw.get('soft'), regs=raw.get('mask_sup'), out=out)
            self._mix(slot)
            self.copied[slot] = self.copy_stream.record_event()

    def _mix(self, slot):
        # the last writer of the slot, on the copy stream: the source slot tensors are only read
        if self.mix is None:
            return
        dmix, roles_s, roles_t, (h, w) = self.mix
        drawn = dmix.draw(h, w)
        if drawn is None:
            return
        dst = self.slots[slot]
        with ops.use_stream(self.copy_stream):
            ops.domain_mix(dst[roles_s['image']], dst[roles_s['mask']], dst[roles_t['image']],
                           label_t=dst.get(roles_t.get('mask')), soft_t=dst.get(roles_t.get('soft')),
                           regs_t=dst.get(roles_t.get('mask_sup')), ignore_label=dmix.ignore_label,
                           class_num=dmix.class_num, flag=self.mix_flag, **{drawn[0]: drawn[1]})

    def next(self):
        """-> the device batch for this step (valid until `release()` + `depth - 1` further `next()` calls); the copy of
        the following batch is started on the copy stream."""
        slot = self.i % len(self.slots)
        torch.cuda.current_stream().wait_event(self.copied[slot])
        self._cur = slot
        if not self.single:
            self._stage(self.i + 1)
        self.i += 1
        return self.slots[slot]

    def release(self, consumed=None):
        """The step consuming the current batch has been enqueued on the current stream.  consumed: an event recorded
        where the step is done READING its inputs (default: the end of everything enqueued so far).  With a single slot
        the copy of the next batch is started here, behind that event."""
        self.consumed[self._cur] = consumed if consumed is not None else torch.cuda.current_stream().record_event()
        if self.single:
            self._stage(self.i)
