"""The exact model of tests/exact_net.py at another depth (tests/test_model_depth.py, tests/test_gpu_depth.py).

exact_net.py reads its module global NB (a copy of synth.NB) in conv_class, make_model and forward, and synth reads its own in
conv_specs / param_text.  depth(nb) sets both for the duration of a `with` block and puts both back whatever happens inside: the
exact-net tests of the default depth run in the same process and must find 23 again.  EVERYTHING that depends on the depth -- making a
model, writing its files, running the mirror -- happens inside the block; no fixture keeps it open across tests.

The committed SEED / GAINS of exact_net.py are chosen for 23 blocks.  At other depths they leave the output one-sided (nb = 1: nothing
above 1; nb = 6: 72 % above 1 on the 50 x 40 frame), so every depth tested here has a (seed, gains) of its own, found by a search over
seeds and trunk gains for models that meet the health conditions of tests/test_exact_net.py (check_health, test_health_tiles) plus
"one changed input pixel changes an output region of at least 16 x 16".  tests/test_model_depth.py asserts that they do.  nb = 2 is
the depth the GPU tests drive through every output path, so its model also meets them on the bgr, RGBA, fp16 and TTA frames -- the TTA
frame with the same model (the committed conv_last gain reaches both clamps there; exact_net.TTA_GAINS is not needed)."""
import contextlib

import exact_net as N
from realsr_ncnn_vulkan_amd import synth

# depth -> (seed, gains over exact_net.GAINS)
MODELS = {
    1: (6, dict(trunk=(0.5, 1.0))),
    2: (34, dict(trunk=(0.5, 1.0))),
    6: (8, dict(trunk=(0.5, 1.0))),
}
MIN_SPREAD = 16  # rows and columns of the output region one input pixel must change


@contextlib.contextmanager
def depth(nb):
    """synth.NB = exact_net.NB = nb inside the block; both restored behind it."""
    old = (synth.NB, N.NB)
    synth.NB = N.NB = int(nb)
    try:
        yield
    finally:
        synth.NB, N.NB = old


def make_model(nb, **gains):
    """The committed exact model of depth nb (call inside depth(nb))."""
    assert synth.NB == N.NB == nb, "build the model inside depth(%d)" % nb
    seed, g = MODELS[nb]
    return N.make_model(seed, **dict(g, **gains))
