"""CPU: derived-state coherence without a GPU (tests/coherence_cases.py).
  (a) transformer.derived() itself on CPU tensors: the identical object while nothing changed; a rebuild after an in-place
      write, a new storage, a dtype change, load_state_dict with and without assign=True; a derived() of derived() values
      follows the innermost parameter; a deep copy gets values of its own;
  (b) the two writes the signature cannot see (``p.data.copy_``, inference-mode parameters) followed by clear_derived() give
      the value of the new weights; clear_derived drops every cache it names; a launch plan refuses a changed model;
  (c) sensitivity: for every family, replacing any one floating state-dict tensor outside its quiet list moves the output of
      the plain-torch float64 CPU form, replacing a listed one does not, and at most 10 % of a family's tensors are listed - so
      no assertion of tests/test_hip_coherence.py can pass vacuously."""
import copy

import pytest
import torch

import coherence_cases as CC
from pytorch_models import transformer as T
from pytorch_models.transformer import clear_derived, derived

torch.set_grad_enabled(False)


def _twice(m):
    """2 w as a derived value of a Linear"""
    return derived(m, "twice", (m.weight, m.bias), lambda: (m.weight.detach().float() * 2).contiguous())


def _lin(seed=1):
    m = torch.nn.Linear(5, 3)
    m.weight.copy_(torch.randn(3, 5, generator=torch.Generator().manual_seed(seed)))
    return m


def _is_twice(m):
    return torch.equal(_twice(m), m.weight.detach().float() * 2)


def test_derived_returns_the_identical_object_while_nothing_changed():
    m = _lin()
    a = _twice(m)
    assert _twice(m) is a and _twice(m) is a
    m.bias.add_(1.0)  # a dependency the value does not even read: still a rebuild
    assert _twice(m) is not a


def test_derived_follows_every_visible_change():
    m = _lin()
    a = _twice(m)
    m.weight.mul_(-0.5)  # in place under no_grad: what a converter's copy_ does
    b = _twice(m)
    assert b is not a and _is_twice(m) and not torch.equal(a, b)
    m.weight.data = torch.ones_like(m.weight)  # a new storage
    assert (_twice(m) == 2).all()
    m.to(torch.bfloat16)  # dtype (and storage)
    c = _twice(m)
    assert c.dtype == torch.float32 and _is_twice(m)
    m.to(torch.float32)
    other = _lin(2)
    m.load_state_dict(other.state_dict())  # copy_ into the parameters
    assert torch.equal(_twice(m), other.weight * 2)
    third = _lin(3)
    m.load_state_dict({k: v.clone() for k, v in third.state_dict().items()}, assign=True)  # new Parameter objects
    assert torch.equal(_twice(m), third.weight * 2)


def test_derived_of_derived_follows_the_innermost_parameter():
    mha = CC.filled(T.MHA(64, 2), 5)
    norm = CC.filled(T.LayerNorm(64), 6)
    wl, s, c = mha._pack_ln(norm)
    assert mha._pack_ln(norm)[0] is wl
    for p in (mha.k_proj.weight, mha.v_proj.bias, norm.weight, norm.bias):
        before = [t.clone() for t in mha._pack_ln(norm)]
        p.add_(0.25)
        after = mha._pack_ln(norm)
        want = T._fold_ln(*mha._pack("qkv"), norm)
        assert all(torch.equal(x, y) for x, y in zip(after, want))
        assert not all(torch.equal(x, y) for x, y in zip(after, before))
    # the inner value rebuilt by a caller that never asks for the outer one (the unfolded path at a small M), twice: the
    # second rebuild may land on the address the outer signature last saw
    mha.q_proj.weight.mul_(2.0)
    mha._pack("qkv")
    mha.q_proj.weight.mul_(2.0)
    mha._pack("qkv")
    assert all(torch.equal(x, y) for x, y in zip(mha._pack_ln(norm), T._fold_ln(*mha._pack("qkv"), norm)))


def test_mbconv_operands_follow_every_batchnorm():
    from pytorch_models.image.maxvit import MBConv

    blk = CC.filled(MBConv(32, 64, 2), 7)

    def flat(t):
        out = []
        for x in t:
            out += flat(x) if isinstance(x, (tuple, list)) else [x]
        return out

    assert blk._packed() is blk._packed()
    for key in CC.float_keys(blk):
        before = [x.clone() for x in flat(blk._packed()) if x is not None]
        CC.overwrite(blk, key)
        got = [x for x in flat(blk._packed()) if x is not None]
        clear_derived(blk)
        want = [x for x in flat(blk._packed()) if x is not None]
        assert all(torch.equal(x, y) for x, y in zip(got, want)), key
        assert not all(torch.equal(x, y) for x, y in zip(got, before)), key  # every tensor of the block is folded into an operand


def test_deepcopy_gets_values_of_its_own():
    m = _lin()
    a = _twice(m)
    twin = copy.deepcopy(m)
    twin.weight.fill_(3.0)
    assert (_twice(twin) == 6).all()
    assert _twice(m) is a and _is_twice(m)
    m.weight.fill_(-1.0)
    assert (_twice(m) == -2).all() and (_twice(twin) == 6).all()


def test_blind_spots_are_served_by_clear_derived():
    # .data writes do not bump _version
    m = _lin()
    _twice(m)
    v = m.weight._version
    m.weight.data.copy_(torch.full_like(m.weight, 4.0))
    assert m.weight._version == v  # the premise: nothing for the signature to see
    clear_derived(m)
    assert (_twice(m) == 8).all()
    # parameters created under inference_mode carry no version counter
    with torch.inference_mode():
        im = torch.nn.Sequential(torch.nn.Linear(5, 3))
        _twice(im[0])
        im[0].weight.fill_(0.5)
        assert im[0].weight.is_inference()
        clear_derived(im)  # through the parent: submodules are covered
        assert (_twice(im[0]) == 1).all()


def test_clear_derived_drops_every_cache_it_names():
    from pytorch_models.text.t5 import RelativePositionBias

    root = torch.nn.Sequential(_lin(), RelativePositionBias(2))
    _twice(root[0])
    root[1](4, True)
    root[1].lut(True)
    root.__dict__["_pm_t5_decode"] = ("key", object())
    root[0].__dict__["_pm_tables"] = {"k": 1}
    assert "_pm_buckets" in root[1].__dict__ and "_pm_derived" in root[1].__dict__
    clear_derived(root)
    for mod in root.modules():
        assert not [k for k in mod.__dict__ if k.startswith("_pm_")], mod
    assert "_pm_derived" not in root.state_dict()


def test_a_launch_plan_refuses_a_changed_model():
    from pytorch_models._hip import decode_plan as plan

    m = torch.nn.Sequential(_lin(), torch.nn.BatchNorm1d(3))
    st = plan.CapturedStep(1, torch.device("cpu"), 4, 1024)
    st.check_model()  # nothing watched: nothing to refuse
    st.watch(m)
    st.check_model()
    m[1].running_mean.add_(1.0)  # a buffer counts
    with pytest.raises(RuntimeError, match="parameters changed.*build a new decoder"):
        st.check_model()
    st.watch(m)
    st.check_model()
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})  # same values, still a write
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.check_model()
    assert T.state_signature(m).sig == T._sig(list(m.parameters()) + list(m.buffers()))  # the fields derived() keys on
    assert T.state_signature(m) == T.state_signature(m)
    m.cpu()  # a module-level move replaces a buffer by a new tensor even where nothing else distinguishes it
    st.watch(m)
    m[1]._buffers["running_var"] = m[1].running_var.clone()
    with pytest.raises(RuntimeError, match="parameters changed"):
        st.check_model()


def test_a_replaced_buffer_is_seen_even_at_the_old_address():
    """module.cpu() / .cuda() replace a buffer by a NEW tensor whose version counter starts again, and an allocator may hand the
    old address back: (address, version, dtype, device) repeats.  Forced here with a tensor over the same memory."""
    m = torch.nn.BatchNorm1d(4)
    mean2 = lambda: derived(m, "mean2", (m.running_mean,), lambda: m.running_mean * 2)  # noqa: E731
    storage = m.running_mean
    for _ in range(4):
        storage.fill_(1.0)
    assert (mean2() == 2).all()
    seen = T._sig((storage,))  # what the cache entry is keyed on
    twin = torch.empty(0).set_(storage.untyped_storage(), 0, storage.shape)  # same address, dtype, device; a version counter of its own
    m._buffers["running_mean"] = twin
    assert twin._version < storage._version
    while twin._version < storage._version:
        twin.add_(1.0)  # ... brought to the same version: now nothing but the object tells the two apart
    assert T._sig((twin,)) == seen and not (twin == 1).any()
    assert torch.equal(mean2(), twin * 2)


# ---- (c) sensitivity
def _cpu_form(fam, model):
    inp = (fam.cpu_inputs or fam.inputs)()
    return fam.cpu(model, inp)


@pytest.mark.parametrize("fid", [f.id for f in CC.FAMILIES.values() if f.cpu is not None])
def test_every_tensor_outside_the_quiet_list_moves_the_output(fid):
    fam = CC.FAMILIES[fid]
    model = fam.make().double()
    keys = fam.keys(model)  # (a family split by submodule: the tensors of this row; the cap holds per row)
    quiet = [k for k in keys if fam.is_quiet(k)]
    assert len(quiet) <= 0.10 * len(keys), (len(quiet), len(keys))  # the cap: a family that needs more is a finding
    for pat in fam.quiet:
        assert any(CC.fnmatch.fnmatchcase(k, pat) for k in keys), f"{pat} matches nothing"
    prev = _cpu_form(fam, model)
    assert prev.dtype == torch.float64 and bool(torch.isfinite(prev).all())
    bad = []
    for key in keys:
        CC.overwrite(model, key)
        out = _cpu_form(fam, model)
        d = CC.change(prev, out)
        if fam.is_quiet(key):
            if not d <= CC.QUIET_MAX:
                bad.append((key, "listed as quiet, moved the output by", d))
        elif not d >= CC.LOUD_MIN:
            bad.append((key, "moved the output by only", d))
        prev = out
    assert not bad, bad


def test_the_table_covers_what_it_claims():
    ids = set(CC.FAMILIES)
    # every family the table was asked to hold: a row dropped from coherence_cases.py fails here
    assert ids == {"encoder_pre", "encoder_post", "decoder_pre_cross", "decoder_post_cross", "encoder_fold", "vit", "mixer_bf16",
                   "mixer_fp32", "convnext", "maxvit", "detr_backbone", "detr_encoder", "detr_decoder", "detr_head", "mobile_vit",
                   "bert", "gpt", "gpt2", "t5", "whisper", "wav2vec2", "hubert", "data2vec_audio", "sew", "ctc", "encodec_encode",
                   "encodec_decode", "spectrogram_power", "spectrogram_mel"}
    want = {"gpt2": {"forward", "generate", "generate_prefill", "score"}, "bert": {"forward", "forward_lengths"},
            "t5": {"forward", "encode_lengths", "generate", "generate_packed", "score"},
            "whisper": {"forward", "generate", "generate_exact", "generate_beams", "align"}, "ctc": {"log_probs", "align"}}
    for fid, names in want.items():
        assert names <= set(CC.FAMILIES[fid].entries), fid
    detr = CC.FAMILIES["detr_backbone"].make()
    split = [k for part in ("backbone", "encoder", "decoder", "head") for k in CC.FAMILIES["detr_" + part].keys(detr)]
    assert sorted(split) == sorted(k for k in CC.float_keys(detr) if k != "pos_embed.freqs")  # the four rows cover DETR, once each
    enc = CC.FAMILIES["encodec_encode"].make()
    assert any("parametrizations.weight" in k for k in CC.float_keys(enc))  # weight-norm parametrizations are present
    assert set(CC.FAMILIES["encodec_encode"].keys(enc)) | set(CC.FAMILIES["encodec_decode"].keys(enc)) == set(CC.float_keys(enc))
    assert sum(f.whole for f in CC.FAMILIES.values() if f.id.startswith("detr_")) == 1
    for fam in CC.FAMILIES.values():
        assert fam.entries and fam.dtype in ("bf16", "fp32")
        if fam.cpu is None:  # no float64 form: nothing may claim that the output moved
            assert not any(e.moves for e in fam.entries.values()), fam.id
        if fam.id.startswith("detr_") and not fam.whole:
            continue  # (the same module as detr_backbone)
        first = fam.make()
        sd, sd2 = CC.named_tensors(first), CC.second_state(fam)
        assert sd.keys() == sd2.keys() and set(first.state_dict()) <= set(sd)
        for k in CC.float_keys(first):
            assert not torch.equal(sd[k], sd2[k]), k  # the second checkpoint differs in every floating tensor
            assert torch.equal(sd2[k], sd2[k].to(torch.bfloat16).float()), k  # and loads into a bf16 module without rounding
        CC.load_state(first, sd2)
        assert all(torch.equal(v, sd2[k]) for k, v in CC.named_tensors(first).items())
    assert set(CC.float_keys(CC.FAMILIES["spectrogram_mel"].make())) == {"window", "filters"}  # the window is no state-dict entry
    assert CC.float_keys(CC.FAMILIES["spectrogram_power"].make()) == ["window"]
