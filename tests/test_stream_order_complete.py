"""Every public method of Context and every ampli_* entry point that takes an ampli_ctx * is either a case of the stream-order suite
(tests/stream_order.py, run by tests/test_gpu_stream_order.py) or exempt from it with a reason: a method added later fails here until
it is placed.  No GPU."""
import os
import re

from tests import stream_order as so


def _public_methods():
    from amplisolve_amd import Context

    return sorted(n for n, f in vars(Context).items() if not n.startswith("_") and (callable(f) or hasattr(f, "__get__")) and n != "LAYOUTS")


def test_every_public_method_is_a_case_or_exempt_with_a_reason():
    from amplisolve_amd import Context

    methods = _public_methods()
    assert len(methods) > 80 and "poisson_call" in methods and "n_calls_total" in methods and "set_ranges" in methods
    in_cases = {m for c in so.cases() for m in c.methods}
    assert in_cases <= set(methods), in_cases - set(methods)
    assert set(so.EXEMPT_METHODS) <= set(methods), set(so.EXEMPT_METHODS) - set(methods)
    assert all(isinstance(r, str) and len(r) > 20 for r in so.EXEMPT_METHODS.values())
    missing = [m for m in methods if m not in in_cases and m not in so.EXEMPT_METHODS]
    assert not missing, f"neither a case of tests/stream_order.py nor exempt: {missing}"
    # what the cases run under the context's stream is what api.py wraps: a method that allocates, fills, uploads or reads back with torch
    unwrapped = [m for m in in_cases if not getattr(vars(Context)[m], "on_stream", False) and m not in so.EXEMPT_OR_PLAIN_IN_CASES]
    assert not unwrapped, f"cases of methods that api.py leaves off the context's stream: {unwrapped}"
    both = sorted(set(so.EXEMPT_METHODS) & in_cases)
    assert not both, f"exempt and a case: {both}"


def test_every_entry_point_with_a_context_is_a_case_or_exempt_with_a_reason():
    protos = so.ctx_prototypes()
    assert len(protos) > 90 and "ampli_poisson_call" in protos and "ampli_pileup_count" in protos and "ampli_ctx_flags" in protos
    in_cases = set()
    for c in so.cases():
        in_cases |= c.entry_points()
    assert set(so.EXEMPT_PROTOS) <= set(protos), set(so.EXEMPT_PROTOS) - set(protos)
    assert all(isinstance(r, str) and len(r) > 20 for r in so.EXEMPT_PROTOS.values())
    missing = [p for p in protos if p not in in_cases and p not in so.EXEMPT_PROTOS]
    assert not missing, f"neither called by a case of tests/stream_order.py nor exempt: {missing}"
    both = sorted(set(so.EXEMPT_PROTOS) & in_cases - so.CALLED_ON_THE_WAY)
    assert not both, f"exempt and called by a case: {both}"


def test_the_case_names_are_unique_and_the_sync_cases_quote_their_line():
    names = [c.name for c in so.cases()]
    assert len(set(names)) == len(names) and len(names) >= 60
    sync = {c.name: c.syncs for c in so.cases() if c.syncs}
    assert set(sync) == {"read_calls", "read_loo_calls", "flags", "pack16", "pack24", "limit_stats", "power_stats", "acc_merge"}, sync
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name, (where, line) in sync.items():
        text = re.sub(r"[\s*]+", " ", open(os.path.join(root, where)).read())  # white space and the comment's leading stars folded
        assert line in text, f"{name}: {where} no longer says {line!r}"
