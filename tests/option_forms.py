"""The option sets of a context (csrc/engine.h, struct Options) that select another device code path for a Krylov step.
One source for the fixed table of tests/test_gpu_option_forms.py and for the draw of tests/fuzz_parity.py; no device work here.

`dia`, `patch`, `reorder` and `stencil` act when an operator is CREATED (capi.hip, engine_core.hip: the stored forms are built then):
a context gets its options first, its operators afterwards -- context_with() is the only way the tests make one."""

OPTION_SETS = {
    "default": {},
    # single-pass step (pipe.hip): the hand-over between steps, how H comes home, where the operator is read from
    "pipeline_serial": {"pipeline_serial": 1},
    "mailbox0": {"mailbox": 0},
    "mailbox0_pipeline_serial": {"mailbox": 0, "pipeline_serial": 1},
    "dia0": {"dia": 0},
    "nontemporal0": {"nontemporal": 0},
    "nontemporal1": {"nontemporal": 1},
    "resident": {"resident": 1},
    "stencil": {"stencil": 1},
    # ... its forms for grids
    "patch1": {"patch": 1},
    "patch1_mailbox0": {"patch": 1, "mailbox": 0},
    "patch0": {"patch": 0},
    "patch0_mailbox0": {"patch": 0, "mailbox": 0},
    "patch0_wave0": {"patch": 0, "wave": 0},
    "patch0_wave0_mailbox0": {"patch": 0, "wave": 0, "mailbox": 0},
    # two-kernel step (fused.hip) and the modular launches, on an operator whose default is the single-pass step
    "pipeline0": {"pipeline": 0},
    "pipeline0_dia0": {"pipeline": 0, "dia": 0},
    "pipeline0_two_reductions": {"pipeline": 0, "fused_two_reductions": 1},
    "pipeline0_fused0": {"pipeline": 0, "fused": 0},
    # two-kernel step on SELL slots (operators without a single-pass form)
    "fa2_pipelined1_reorder0": {"fa2_pipelined": 1, "reorder": 0},
    "fa2_pipelined0_reorder0": {"fa2_pipelined": 0, "reorder": 0},
    # (rows whose columns stay within a few tiles take the wave form of the single-pass step on SELL slots for the real types:
    #  pipeline = 0 is what sends them through the two-kernel step's first kernel, like tools/fa2_check.py does)
    "fa2_pipelined1_reorder0_pipeline0": {"fa2_pipelined": 1, "reorder": 0, "pipeline": 0},
    "fa2_pipelined0_reorder0_pipeline0": {"fa2_pipelined": 0, "reorder": 0, "pipeline": 0},
    "two_reductions": {"fused_two_reductions": 1},
    "fused0": {"fused": 0},
    "reorder2": {"reorder": 2},
    # kiops after a rejected sub-step / the batched step's resident rounds
    "kiops_skip_redo0": {"kiops_skip_redo": 0},
    "batch_rounds1": {"batch_rounds": 1},
    "batch_rounds3": {"batch_rounds": 3},
    "batch_rounds7": {"batch_rounds": 7},
}

# sizes at which test_resident_form_matches_stepwise_and_oracle runs the resident kernel (one cooperative launch: the fuzzer keeps to them)
RESIDENT_SIZES = (4096, 70_001, 200_000)


def context_with(eu, options, **kw):
    """a private context with `options` set -- before any operator exists on it"""
    ctx = eu.Context(**kw)
    for name, value in options.items():
        ctx.set_option(name, value)
        assert ctx.get_option(name) == value, (name, value)
    return ctx
