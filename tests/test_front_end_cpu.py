"""The argument handling of every public VAR call on a CPU model against tests/golden/front_end.json (tests/frontcases.py): which arguments
are refused and with which words, what reaches the engine, what the PyTorch paths return."""
from tests import frontcases


def test_front_end_cpu():
    outcomes, _ = frontcases.record('cpu')
    same, moved = frontcases.compare('cpu', outcomes)
    print(same, 'cases as recorded,', moved, 'in UNIFIED')


def test_unified_cases_follow_the_rules():
    """a changed case is a refusal that became a ValueError, a bool that is refused now, or a numpy integer label that is accepted now"""
    for section, table in frontcases.UNIFIED.items():
        for case, (then, now) in table.items():
            assert then != now, case
            if now[0] == 'raise':
                assert now[1] == 'ValueError', case
                assert then[0] == 'raise' and then[1:] != now[1:] or '=True' in case or '=False' in case, case
            else:
                assert then[0] == 'raise' and 'np.int' in case and 'label' in case, case
