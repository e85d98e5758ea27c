"""The launch order of the four whole-picture steps (stages.FramePipeline, BFramePipeline, MultiRefFramePipeline, IFramePipeline),
without the library and without a device: hipabi.lib is replaced by a recorder whose every entry logs its name, torch.cuda's streams
and events by stand-ins that log the stream an entry was issued on and every wait edge, and `mark` logs "#name".  The expected logs
are literals, recorded with this recorder when every step still carried its own copy of the loop-filter tail.  What is
asserted: the order of the entries, their streams, the wait edges and the marks - nothing about arguments or results."""
import contextlib
import importlib

import numpy as np
import pytest
import torch

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")

SWITCHES = ("X265HIP_PAR_SCHEDULE", "X265HIP_FUSE_SAO", "X265HIP_LA_AFTER_ME", "X265HIP_PREP_OVERLAP", "X265HIP_SUBPEL_DEFER",
            "X265HIP_BORDER_PLANES")


class Recorder:
    """The stand-in for the library (`lib`), for torch.cuda's streams and events, and the `mark` of a step: everything lands in `log`."""

    def __init__(self):
        self.log, self.main, self.made, self.with_streams = [], Stream(self, "main"), 0, False
        self.cur = [self.main]
        self.lib = Lib(self)

    def entry(self, name):
        self.log.append((self.cur[-1].name + ":" if self.with_streams else "") + name)

    def mark(self, name):
        self.log.append("#" + name)

    def new_stream(self, *a, **kw):
        self.made += 1
        return Stream(self, "s%d" % self.made)

    @contextlib.contextmanager
    def stream(self, s):
        self.cur.append(s)
        try:
            yield
        finally:
            self.cur.pop()

    def take(self):
        out, self.log = " ".join(self.log), []
        return out


class Lib:
    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        def call(*args):
            self._rec.entry(name[len("x265hip_"):])
            return 64 if name.endswith("_scratch_bytes") else 3 if name.endswith("_waves") else 0
        call.argtypes = call.restype = None
        setattr(self, name, call)
        return call


class Stream:
    cuda_stream = 0

    def __init__(self, rec, name):
        self.rec, self.name = rec, name

    def wait_event(self, ev):
        self.rec.log.append("%s<-ev@%s" % (self.name, ev.on))

    def wait_stream(self, s):
        self.rec.log.append("%s<-ev@%s" % (self.name, s.name))


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()

    class Event:
        def record(self, stream=None):
            self.on = (stream or r.cur[-1]).name
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(A, "lib", lambda: r.lib)
    monkeypatch.setattr(A, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "Stream", r.new_stream)
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(torch.cuda, "stream", r.stream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: r.cur[-1])
    return r


def picture(w=128, h=64):
    return P.DevicePicture(np.zeros((h, w), np.uint8), "cpu", np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8))


RDO = dict(lambdas=(1, 1), ctx_merge=0, ctx_type=0, entropy_bits=np.zeros(128, np.uint32))
OPTIONS = {"rdo": dict(deblock=True, sao=True, chroma=True, sao_apply=True, sao_rdo=RDO),
           "standin": dict(deblock=True, sao=True, chroma=True, sao_apply=True),
           "noapply": dict(deblock=True, sao=True, chroma=True),
           "nochroma": dict(deblock=True, sao=True, sao_apply=True),
           "none": {}}
PARALLEL = dict(OPTIONS["rdo"], parallel_planes=True, subpel_planes=True, lookahead=(128, 64))


def two_runs(rec, monkeypatch, step, opts, env=(), size=(128, 64), band=None, marks=True):
    """The logs of two run() calls of a freshly built step."""
    for k, v in env:
        monkeypatch.setenv(k, v)
    w, h = size
    cur, ref, ref2 = picture(w, h), picture(w, h), picture(w, h)
    if step == "P":
        pipe, args = S.FramePipeline(w, h, 8, "cpu", rng=8, level=2, **opts), (cur, ref)
        pipe.band_border = band
    elif step == "B":
        pipe, args = S.BFramePipeline(w, h, 8, "cpu", rng=8, level=2, **opts), (cur, ref, ref2)
    elif step == "M":
        pipe, args = S.MultiRefFramePipeline(w, h, 8, "cpu", max_refs=2, rng=8, level=2, **opts), (cur, [ref, ref2])
    else:
        pipe, args = S.IFramePipeline(w, h, 8, "cpu", level=2, **opts), (cur,)
    rec.take()                      # what the constructor asked the library (scratch sizes, waves) is not a launch of the step
    rec.with_streams = not marks
    logs = []
    for _ in range(2):
        pipe.run(*args, mark=rec.mark if marks else None)
        logs.append(rec.take())
    return logs


# (step, option set) -> the log of one run() at 128x64, 8 bit, range 8, level 2 (M: two references)
SERIAL = {
    ("P", "rdo"):
        "me_best_reset #lookahead me_fullsearch #me subpel_refine #subpel inter_recon #recon inter_recon_chroma_pair "
        "#recon_chroma deblock_bs_inter deblock_luma deblock_chroma #deblock sao_planes #sao_stats sao_rdo #sao_rdo "
        "sao_apply_planes #sao_apply extend_border_planes #border",
    ("P", "standin"):
        "me_best_reset #lookahead me_fullsearch #me subpel_refine #subpel inter_recon #recon inter_recon_chroma_pair "
        "#recon_chroma deblock_bs_inter deblock_luma deblock_chroma #deblock sao_planes #sao extend_border_planes "
        "#border",
    ("P", "noapply"):
        "me_best_reset #lookahead me_fullsearch #me subpel_refine #subpel inter_recon #recon inter_recon_chroma_pair "
        "#recon_chroma deblock_bs_inter deblock_luma deblock_chroma #deblock sao_stats sao_stats sao_stats #sao_stats "
        "extend_border_planes #border",
    ("P", "nochroma"):
        "me_best_reset #lookahead me_fullsearch #me subpel_refine #subpel inter_recon #recon deblock_bs_inter "
        "deblock_luma #deblock sao_stats #sao_stats sao_decide sao_apply #sao_apply extend_border_planes #border",
    ("P", "none"):
        "me_best_reset #lookahead me_fullsearch #me subpel_refine #subpel inter_recon #recon extend_border_planes "
        "#border",
    ("B", "rdo"):
        "me_best_reset me_fullsearch #me0 subpel_refine #subpel0 me_best_reset me_fullsearch #me1 subpel_refine "
        "#subpel1 bidir_decide #bidir inter_recon_bi #recon inter_recon_chroma_bi inter_recon_chroma_bi #recon_chroma "
        "deblock_bs_inter deblock_luma deblock_chroma #deblock sao_planes #sao_stats sao_rdo #sao_rdo sao_apply_planes "
        "#sao_apply extend_border_planes #border",
    ("B", "standin"):
        "me_best_reset me_fullsearch #me0 subpel_refine #subpel0 me_best_reset me_fullsearch #me1 subpel_refine "
        "#subpel1 bidir_decide #bidir inter_recon_bi #recon inter_recon_chroma_bi inter_recon_chroma_bi #recon_chroma "
        "deblock_bs_inter deblock_luma deblock_chroma #deblock sao_stats sao_stats sao_stats #sao_stats sao_decide "
        "sao_apply sao_decide sao_apply sao_decide sao_apply #sao_apply extend_border_planes #border",
    ("B", "noapply"):
        "me_best_reset me_fullsearch #me0 subpel_refine #subpel0 me_best_reset me_fullsearch #me1 subpel_refine "
        "#subpel1 bidir_decide #bidir inter_recon_bi #recon inter_recon_chroma_bi inter_recon_chroma_bi #recon_chroma "
        "deblock_bs_inter deblock_luma deblock_chroma #deblock sao_stats sao_stats sao_stats #sao_stats "
        "extend_border_planes #border",
    ("B", "nochroma"):
        "me_best_reset me_fullsearch #me0 subpel_refine #subpel0 me_best_reset me_fullsearch #me1 subpel_refine "
        "#subpel1 bidir_decide #bidir inter_recon_bi #recon deblock_bs_inter deblock_luma #deblock sao_stats #sao_stats "
        "sao_decide sao_apply #sao_apply extend_border_planes #border",
    ("B", "none"):
        "me_best_reset me_fullsearch #me0 subpel_refine #subpel0 me_best_reset me_fullsearch #me1 subpel_refine "
        "#subpel1 bidir_decide #bidir inter_recon_bi #recon extend_border_planes #border",
    ("M", "rdo"):
        "me_best_reset me_fullsearch #me0 subpel_refine #subpel0 me_best_reset me_fullsearch #me1 subpel_refine "
        "#subpel1 ref_select #ref_select inter_recon_refs #recon inter_recon_chroma_pair_refs #recon_chroma "
        "deblock_bs_inter deblock_luma deblock_chroma #deblock sao_planes #sao_stats sao_rdo #sao_rdo sao_apply_planes "
        "#sao_apply extend_border_planes #border",
    ("M", "standin"):
        "me_best_reset me_fullsearch #me0 subpel_refine #subpel0 me_best_reset me_fullsearch #me1 subpel_refine "
        "#subpel1 ref_select #ref_select inter_recon_refs #recon inter_recon_chroma_pair_refs #recon_chroma "
        "deblock_bs_inter deblock_luma deblock_chroma #deblock sao_stats sao_stats sao_stats #sao_stats sao_decide "
        "sao_apply sao_decide sao_apply sao_decide sao_apply #sao_apply extend_border_planes #border",
    ("M", "noapply"):
        "me_best_reset me_fullsearch #me0 subpel_refine #subpel0 me_best_reset me_fullsearch #me1 subpel_refine "
        "#subpel1 ref_select #ref_select inter_recon_refs #recon inter_recon_chroma_pair_refs #recon_chroma "
        "deblock_bs_inter deblock_luma deblock_chroma #deblock sao_stats sao_stats sao_stats #sao_stats "
        "extend_border_planes #border",
    ("M", "nochroma"):
        "me_best_reset me_fullsearch #me0 subpel_refine #subpel0 me_best_reset me_fullsearch #me1 subpel_refine "
        "#subpel1 ref_select #ref_select inter_recon_refs #recon deblock_bs_inter deblock_luma #deblock sao_stats "
        "#sao_stats sao_decide sao_apply #sao_apply extend_border_planes #border",
    ("M", "none"):
        "me_best_reset me_fullsearch #me0 subpel_refine #subpel0 me_best_reset me_fullsearch #me1 subpel_refine "
        "#subpel1 ref_select #ref_select inter_recon_refs #recon extend_border_planes #border",
    ("I", "rdo"):
        "intra_picture #intra deblock_bs_inter deblock_luma deblock_chroma #deblock sao_planes #sao_stats sao_rdo "
        "#sao_rdo sao_apply_planes #sao_apply extend_border_planes #border",
    ("I", "standin"):
        "intra_picture #intra deblock_bs_inter deblock_luma deblock_chroma #deblock sao_stats sao_stats sao_stats "
        "#sao_stats sao_decide sao_apply sao_decide sao_apply sao_decide sao_apply #sao_apply extend_border_planes "
        "#border",
    ("I", "noapply"):
        "intra_picture #intra deblock_bs_inter deblock_luma deblock_chroma #deblock sao_stats sao_stats sao_stats "
        "#sao_stats extend_border_planes #border",
    ("I", "nochroma"):
        "intra_picture #intra deblock_bs_inter deblock_luma #deblock sao_stats #sao_stats sao_decide sao_apply "
        "#sao_apply extend_border_planes #border",
    ("I", "none"):
        "intra_picture #intra extend_border_planes #border",
}

_P_HEAD = ("me_best_reset #lookahead me_fullsearch #me subpel_refine #subpel inter_recon #recon inter_recon_chroma_pair "
           "#recon_chroma deblock_bs_inter deblock_luma deblock_chroma #deblock ")
_PAR2 = ("main:me_best_reset main:me_fullsearch main:phase_planes main:subpel_refine_levels main:inter_recon s1<-ev@main "
         "s1:inter_recon_chroma_pair main:deblock_bs_inter main:deblock_luma s1<-ev@main s1:deblock_chroma s1:sao_planes "
         "s1:me_best_reset s1:lowres_init s1:lowres_intra s1:subpel_refine_levels main:sao_planes main<-ev@s1 "
         "main:sao_rdo main:sao_apply_planes ")
_PAR2_NODEFER = ("main:me_best_reset main:me_fullsearch main:phase_planes main:subpel_refine main:inter_recon s1<-ev@main "
                 "s1:inter_recon_chroma_pair main:deblock_bs_inter main:deblock_luma s1<-ev@main s1:deblock_chroma s1:sao_planes "
                 "s1:me_best_reset s1:lowres_init s1:lowres_intra main:sao_planes main<-ev@s1 main:sao_rdo main:sao_apply_planes "
                 "main:extend_border_planes main<-ev@s1")
# the round-2 schedule up to the chroma deblocking, in one piece and in two parts
_PAR1_HEAD = ("main:me_best_reset main:me_fullsearch s3<-ev@main s3:lowres_init s3:lowres_intra main:phase_planes "
              "main:subpel_refine main:inter_recon s1<-ev@main s1:inter_recon_chroma s2<-ev@main s2:inter_recon_chroma "
              "main:deblock_bs_inter main:deblock_luma s1<-ev@main s1<-ev@s2 s1:deblock_chroma s2<-ev@s1 ")
_SPLIT2_HEAD = ("s3<-ev@main s3:lowres_init s3:lowres_intra main:me_best_reset s4<-ev@main s4:phase_planes main:me_fullsearch "
                "s4<-ev@main s4:subpel_refine s4:inter_recon s1<-ev@s4 s1:inter_recon_chroma s2<-ev@s4 s2:inter_recon_chroma "
                "main:me_fullsearch main<-ev@s4 main:subpel_refine main:inter_recon s1<-ev@main s1:inter_recon_chroma "
                "s2<-ev@main s2:inter_recon_chroma main:deblock_bs_inter main:deblock_luma s1<-ev@main s1<-ev@s2 "
                "s1:deblock_chroma s2<-ev@s1 ")
_PAR1_RDO = "main:sao_stats s1:sao_stats s2:sao_stats main<-ev@s1 main<-ev@s2 main:sao_rdo main:sao_apply_planes "
_PAR1_BORDERS = "main:extend_border s1<-ev@main s1:extend_border s2<-ev@main s2:extend_border main<-ev@s1 main<-ev@s2 main<-ev@s3"
_RESET = "main:me_best_reset "          # the second run of the default schedule takes the minima the first cleared on the side stream
_STANDIN, _BAND = OPTIONS["standin"], (True, False)

# (id, arguments of two_runs, log of the first run, log of the second run or None = the same)
EXTRA = [
    ("P-standin-band", dict(step="P", opts=_STANDIN, band=_BAND), _P_HEAD + "sao_planes #sao extend_border_planes #border", None),
    ("P-standin-band-border3", dict(step="P", opts=_STANDIN, band=_BAND, env=(("X265HIP_BORDER_PLANES", "0"),)),
     _P_HEAD + "sao_planes #sao extend_border_rows extend_border_rows extend_border_rows #border", None),
    ("P-standin-border3", dict(step="P", opts=_STANDIN, env=(("X265HIP_BORDER_PLANES", "0"),)),
     _P_HEAD + "sao_planes #sao extend_border extend_border extend_border #border", None),
    ("P-standin-nofuse", dict(step="P", opts=_STANDIN, env=(("X265HIP_FUSE_SAO", "0"),)),
     _P_HEAD +"sao_stats sao_stats sao_stats #sao_stats sao_decide sao_apply sao_decide sao_apply sao_decide sao_apply #sao_apply "
     "extend_border_planes #border", None),
    ("P-parallel2", dict(step="P", opts=PARALLEL, marks=False),
     _PAR2 + "main:extend_border_planes main<-ev@s1", (_PAR2 + "main:extend_border_planes main<-ev@s1")[len(_RESET):]),
    ("P-parallel2-border3", dict(step="P", opts=PARALLEL, marks=False, env=(("X265HIP_BORDER_PLANES", "0"),)),
     _PAR2 + "main:extend_border main:extend_border main:extend_border main<-ev@s1",
     (_PAR2 + "main:extend_border main:extend_border main:extend_border main<-ev@s1")[len(_RESET):]),
    ("P-parallel2-nodefer", dict(step="P", opts=PARALLEL, marks=False, env=(("X265HIP_SUBPEL_DEFER", "0"),)),
     _PAR2_NODEFER, _PAR2_NODEFER[len(_RESET):]),
    ("P-parallel1", dict(step="P", opts=PARALLEL, marks=False, env=(("X265HIP_PAR_SCHEDULE", "1"),)),
     _PAR1_HEAD + _PAR1_RDO + _PAR1_BORDERS, None),
    ("P-parallel1-band", dict(step="P", opts=PARALLEL, marks=False, band=(False, True)),
     _PAR1_HEAD + _PAR1_RDO + _PAR1_BORDERS.replace("extend_border", "extend_border_rows"), None),
    ("P-parallel1-standin", dict(step="P", opts=dict(PARALLEL, sao_rdo=None), marks=False),
     _PAR1_HEAD + "main:sao_stats main:sao_decide main:sao_apply main:extend_border s1:sao_stats s1:sao_decide s1:sao_apply s1:extend_border "
     "s2:sao_stats s2:sao_decide s2:sao_apply s2:extend_border main<-ev@s1 main<-ev@s2 main<-ev@s3", None),
    ("P-parallel1-standin-fuse2", dict(step="P", opts=dict(PARALLEL, sao_rdo=None), marks=False, env=(("X265HIP_FUSE_SAO", "2"),)),
     _PAR1_HEAD + "main<-ev@s1 main:sao_planes " + _PAR1_BORDERS, None),
    ("P-parallel-split2", dict(step="P", opts=dict(PARALLEL, split=2, lookahead=(128, 128)), marks=False, size=(128, 128)),
     _SPLIT2_HEAD + _PAR1_RDO + _PAR1_BORDERS, None),
]


def all_cases():
    for (step, o), want in SERIAL.items():
        yield pytest.param(dict(step=step, opts=OPTIONS[o]), want, None, id="%s-%s" % (step, o))
    for name, kw, want, want2 in EXTRA:
        yield pytest.param(kw, want, want2, id=name)


@pytest.mark.parametrize("kw,want,want2", all_cases())
def test_a_step_launches_what_it_launched_before_the_tail_was_shared(rec, monkeypatch, kw, want, want2):
    first, second = two_runs(rec, monkeypatch, **kw)
    assert first == want
    assert second == (want if want2 is None else want2)         # allocation on first use is not a launch
