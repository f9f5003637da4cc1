"""--diffaug: differentiable augmentation of everything the discriminators see (DiffAugment, Zhao et al. 2020).  The same
family of random transforms -- brightness, contrast about the mean, translation with zero fill, cutout -- goes over the real and the
fake tensor of every discriminator call, and the generator's gradient flows back through the transform.  Not in the reference.

DiffAugment owns what the option needs on the device: the policy, the ratios, the colour mask of the discriminator input, the Philox
key and offset of the parameter stream (a stream of its own: the latent and dropout streams draw what they draw without the option)
and the record buffer.  Saturation is left out: it needs two colour channels, and these images have one."""
import torch

from . import ops

OPERATIONS = ('translation', 'cutout', 'brightness', 'contrast')
SUPPORTED_MODELS = ('fcgan', 'cgan', 'cgan2', 'segmentation')
STREAM_KEY = 7919      # the parameter stream's Philox key is the trainer's seed + this, as 977 marks the conditional trainers' latent


def parse_policy(text):
    """'translation,cutout,color' -> the operations in DiffAugment's order; `color` is brightness and contrast.  An unknown name,
    or an empty list, raises ValueError."""
    names = [n.strip() for n in str(text).split(',') if n.strip()]
    if not names:
        raise ValueError("--diffaug: a comma list of %s, or color (= brightness,contrast)" % ', '.join(OPERATIONS))
    want = set()
    for n in names:
        if n == 'color':
            want.update(('brightness', 'contrast'))
        elif n in OPERATIONS:
            want.add(n)
        else:
            raise ValueError("--diffaug: unknown operation '%s'; choose from %s, or color (= brightness,contrast)" % (n, ', '.join(OPERATIONS)))
    return tuple(op for op in OPERATIONS if op in want)


def policy_bits(policy):
    return sum(ops.DIFFAUG_BITS[op] for op in policy)


def colour_mask(letters, colour_letters):
    """Bit p set where position p of the discriminator input is a colour channel.  letters: the RGB letter behind every channel of
    that input in order, None for a channel that is no image channel (a class score)."""
    return sum(1 << p for p, c in enumerate(letters) if c is not None and c in colour_letters)


def input_letters(opt):
    """The letter behind every channel of the discriminator input of --model opt.model, from --which_channel and --no_cgan."""
    parts = opt.which_channel.split('_')
    if opt.model == 'fcgan':
        return [c for s in parts for c in s]
    a, b = parts
    if opt.model == 'segmentation':      # the generator emits one score per class: no image channel among them
        n = len(b) + (1 if getattr(opt, 'add_background_onehot', False) else 0)
        b = [None] * n
    return list(b) if opt.no_cgan else list(a) + list(b)


def check_options(opt):
    """What --diffaug asks of the other options, refused before anything is built; leaves the parsed policy in opt.diffaug_policy
    (None without the option).  An options object without the flag (the test drivers) passes."""
    text = getattr(opt, 'diffaug', None)
    opt.diffaug_policy = None
    if text is None:
        return
    policy = parse_policy(text)
    if getattr(opt, 'model', None) not in SUPPORTED_MODELS:
        raise ValueError("--diffaug augments the discriminator inputs of --model %s; --model %s is not among them"
                         % (', '.join(SUPPORTED_MODELS), getattr(opt, 'model', None)))
    if getattr(opt, 'which_model_netD', None) == 'None':
        raise ValueError("--diffaug with --which_model_netD None: there is no discriminator input to augment")
    for name in ('diffaug_translation', 'diffaug_cutout'):
        v = getattr(opt, name)
        if not 0.0 <= v <= 1.0:      # a NaN fails both comparisons
            raise ValueError("--%s: a ratio of 0 .. 1 (got %g)" % (name, v))
    if any(c not in 'rgb' for c in opt.diffaug_color_channels):
        raise ValueError("--diffaug_color_channels: letters of r, g, b (got '%s')" % opt.diffaug_color_channels)
    if ('brightness' in policy or 'contrast' in policy) and colour_mask(input_letters(opt), opt.diffaug_color_channels) == 0:
        raise ValueError("--diffaug %s: none of the channels '%s' (--diffaug_color_channels) is in the discriminator input of --model %s "
                         "--which_channel %s%s; drop the colour operations or name the image channel"
                         % (text, opt.diffaug_color_channels, opt.model, opt.which_channel, ' --no_cgan' if opt.no_cgan else ''))
    opt.diffaug_policy = policy


class DiffAugment:
    """augment([t0, t1, ...], slot): draws one record per tensor into records[slot ...] and returns the transformed tensors; every
    launch is enqueued on the current stream and the offset lives on the device, so the call captures into the graphed step and
    every replay draws afresh.  A stage keeps its slots to itself: the records stay in place for its backward."""
    SLOTS = 4      # D stage: slots 0, 1 (pooled fake, real); G stage: slot 2

    def __init__(self, policy, rt, rc, mask, seed, device):
        self.policy = tuple(policy)
        self.policy_bits = policy_bits(self.policy)
        self.rt, self.rc = float(rt), float(rc)
        self.colour_mask = int(mask)
        self.seed = int(seed) + STREAM_KEY
        self.offset = torch.zeros(1, dtype=torch.int64, device=device)
        self.records = torch.zeros((self.SLOTS, 8), dtype=torch.int32, device=device)
        self.workspace = ops.diffaug_workspace(ops.DIFFAUG_MAX_JOBS, device) if 'contrast' in self.policy else None

    @classmethod
    def from_options(cls, opt, seed, device):
        return cls(opt.diffaug_policy, opt.diffaug_translation, opt.diffaug_cutout,
                   colour_mask(input_letters(opt), opt.diffaug_color_channels), seed, device)

    def augment(self, tensors, slot=0):
        assert slot + len(tensors) <= self.SLOTS
        ops.diffaug_draw(self.records[slot: slot + len(tensors)], [tuple(t.shape[2:]) for t in tensors], self.policy_bits, self.rt, self.rc,
                         self.seed, self.offset)
        return ops.diffaug(list(tensors), self, slot)
