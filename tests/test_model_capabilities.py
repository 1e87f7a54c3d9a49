"""What each model kind is allowed to do, read through the C ABI with dummy pointers: every check here runs before any HIP call (as in
test_abi.py::test_argument_validation_of_the_step_entry_points), so no GPU is needed.  The rules live in the rows of the table by kind
(csrc/host_util.h::Family): the descriptor check of a family, whether it has a split backward, a hidden context, a raw hidden context."""
import ctypes

import pytest

from ardae_amd import _lib as L

SOFTPLUS, ELU = 2, 3
NUMBERS = range(-1, 14)
UNKNOWN = (-1, 10, 13)
IMPLICIT, GAUSS = (0, 1, 2, 3, 4, 5, 6, 7), (8, 9, 11, 12)
CLIP = (1 << L.MODEL_CLIP_Z0_SHIFT) | (6 << L.MODEL_CLIP_Z_SHIFT)
HEAD = 2 << L.MODEL_HEAD_SHIFT

one = ctypes.c_void_p(64)            # any non-null address: validation must answer before it is dereferenced
big = ctypes.c_size_t(1 << 40)


def desc(kind, flags=0):
    """The smallest valid descriptor of a kind (an unknown number gets the MLP's dimensions)."""
    if kind in (2, 4):
        return L.ModelDesc(kind, 784, 10, 800, 8, 1, SOFTPLUS, flags)
    if kind in (5, 6):
        return L.ModelDesc(kind, 784, 10, 40, 8, 1, ELU, flags)
    if kind == 11:
        return L.ModelDesc(kind, 784, 0, 800, 8, 1, SOFTPLUS, flags)
    if kind == 12:
        return L.ModelDesc(kind, 784, 0, 40, 8, 1, ELU, flags)
    return L.ModelDesc(kind, 24, 0 if kind in (8, 9) else 10, 64, 8, 2, SOFTPLUS, flags)


def answer(rc):
    assert rc < 0
    return L.lib().ardae_last_error().decode()


def accepted(kind, flags):
    return L.lib().ardae_model_param_floats(ctypes.byref(desc(kind, flags))) != 0


def test_the_smallest_descriptors_are_valid():
    lib = L.lib()
    for k in IMPLICIT + GAUSS:
        d = desc(k)
        assert lib.ardae_model_param_floats(ctypes.byref(d)) > 0 and lib.ardae_model_packed_floats(ctypes.byref(d)) > 0, k
        assert lib.ardae_model_workspace_floats(ctypes.byref(d), 3, 1, 1) > 0, k


@pytest.mark.parametrize("kind", UNKNOWN)
def test_unknown_kinds_are_refused_everywhere(kind):
    lib = L.lib()
    d = desc(kind)
    assert lib.ardae_model_param_floats(ctypes.byref(d)) == 0
    assert lib.ardae_model_packed_floats(ctypes.byref(d)) == 0
    for mode in range(4):
        assert lib.ardae_model_workspace_floats(ctypes.byref(d), 3, 1, mode) == 0
    assert "kind must be" in answer(lib.ardae_model_pack(ctypes.byref(d), one, one, None))
    # ... and by the entry points below, with the same message: the kind is checked before any capability
    assert "kind must be" in answer(lib.ardae_model_vae_backward_decoder(ctypes.byref(d), one, one, one, one, 3, 1, 1.0, 1.0, one, big, None))
    assert "kind must be" in answer(lib.ardae_model_vae_backward_sampler(ctypes.byref(d), one, one, one, one, 3, 1, one, 1.0, one, big, one, 0.0, None))
    assert "kind must be" in answer(lib.ardae_model_encode_hidden(ctypes.byref(d), one, one, one, 3, one, big, one, None, None))
    assert "kind must be" in answer(lib.ardae_model_encode_hidden_raw(ctypes.byref(d), one, one, one, None, 3, one, big, None, None, None))


def test_the_split_backward_is_the_mlp_familys():
    """Every kind but 0 and 1 is refused.  (Kinds 0 / 1 pass the check and go on to launch, which dummy pointers cannot show: their split backward
    runs on the device in the engine's tests.)"""
    lib = L.lib()
    for k in NUMBERS:
        if k in UNKNOWN or k in (0, 1):
            continue
        d = desc(k)
        assert "no split backward" in answer(lib.ardae_model_vae_backward_decoder(ctypes.byref(d), one, one, one, one, 3, 1, 1.0, 1.0, one, big, None)), k
        assert "no split backward" in answer(
            lib.ardae_model_vae_backward_sampler(ctypes.byref(d), one, one, one, one, 3, 1, one, 1.0, one, big, one, 0.0, None)), k


def test_the_hidden_context_is_the_aux_models():
    """hidden_out NULL is the argument check AFTER the capability check: kinds 3, 4, 6, 7 reach it, every other kind is stopped before."""
    lib = L.lib()
    for k in NUMBERS:
        if k in UNKNOWN:
            continue
        msg = answer(lib.ardae_model_encode_hidden(ctypes.byref(desc(k)), one, one, one, 3, one, big, one, None, None))
        assert ("hidden_out is NULL" if k in (3, 4, 6, 7) else "hidden1a context") in msg, (k, msg)


def test_the_raw_hidden_context_is_the_clipped_aux_resconv_class():
    """Both outputs NULL is the argument check after the capability check: only kind 6 with ARDAE_MODEL_CLIPPED reaches it."""
    lib = L.lib()

    def raw(d):
        return answer(lib.ardae_model_encode_hidden_raw(ctypes.byref(d), one, one, one, None, 3, one, big, None, None, None))

    assert "nothing to return" in raw(desc(6, L.MODEL_CLIPPED))
    assert "nothing to return" in raw(desc(6, L.MODEL_CLIPPED | L.MODEL_NO_CENTER))
    for k in NUMBERS:
        if k not in UNKNOWN:
            assert "clipped aux-resconv class only" in raw(desc(k)), k


def test_flag_rules_of_the_descriptor_check():
    for k in IMPLICIT + GAUSS:
        # the log-variance clip codes: kinds 3 / 7
        assert accepted(k, CLIP) == (k in (3, 7)), k
        assert accepted(k, 10 << L.MODEL_CLIP_Z0_SHIFT) == (k in (3, 7)), k
        assert accepted(k, 10 << L.MODEL_CLIP_Z_SHIFT) == (k in (3, 7)), k
        assert not accepted(k, 11 << L.MODEL_CLIP_Z0_SHIFT) and not accepted(k, 11 << L.MODEL_CLIP_Z_SHIFT), k     # a code above 10: nowhere
        assert not accepted(k, CLIP | L.MODEL_NO_CENTER), k
        # ARDAE_MODEL_NO_CENTER: the residual-conv kinds (5 / 6 and the baseline, kind 12)
        assert accepted(k, L.MODEL_NO_CENTER) == (k in (5, 6, 12)), k
        # the sampler-head bits: kind 5, codes 0 .. 4
        for code in (1, 2, 3, 4):
            assert accepted(k, code << L.MODEL_HEAD_SHIFT) == (k == 5), (k, code)
            assert accepted(k, (code << L.MODEL_HEAD_SHIFT) | L.MODEL_NO_CENTER) == (k == 5), (k, code)
        for code in (5, 6, 7):
            assert not accepted(k, code << L.MODEL_HEAD_SHIFT), (k, code)
        # ARDAE_MODEL_CLIPPED: kind 6
        assert accepted(k, L.MODEL_CLIPPED) == (k == 6), k
        assert accepted(k, L.MODEL_CLIPPED | L.MODEL_NO_CENTER) == (k == 6), k
        assert not accepted(k, L.MODEL_CLIPPED | HEAD), k
        # a bit no kind knows
        assert not accepted(k, 32) and not accepted(k, 1 << 16), k
    # kinds 0 / 1 / 2 / 4 take no flag at all
    for k in (0, 1, 2, 4):
        for bit in range(17):
            assert not accepted(k, 1 << bit), (k, bit)


def test_a_refused_descriptor_is_refused_by_every_size_query_and_by_pack():
    lib = L.lib()
    for k, flags in ((0, 1), (2, CLIP), (3, L.MODEL_CLIPPED), (4, HEAD), (5, L.MODEL_CLIPPED), (5, 5 << L.MODEL_HEAD_SHIFT), (6, HEAD), (7, 1)):
        d = desc(k, flags)
        assert lib.ardae_model_param_floats(ctypes.byref(d)) == 0 and lib.ardae_model_packed_floats(ctypes.byref(d)) == 0, (k, flags)
        assert lib.ardae_model_workspace_floats(ctypes.byref(d), 3, 1, 1) == 0, (k, flags)
        assert lib.ardae_model_pack(ctypes.byref(d), one, one, None) < 0, (k, flags)
