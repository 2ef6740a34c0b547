"""Every flag combination around --loss, --berhu-fraction and --loss-gradient that the training driver and the evaluation
driver refuse: the exit code and the refusal that reaches stdout and stderr are those recorded in
tests/golden/objective_refusals.json before the refusals were written once per driver, byte for byte.  What is not the
refusal is left out on both sides: a log line's time stamp, the DEBUG and INFO lines before it (one of them prints every
flag the driver has) and argparse's usage block.  All of them are refused before anything touches a GPU."""
import contextlib
import io
import json
import os
import re
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'objective_refusals.json')
CASES = json.load(open(GOLDEN))
STAMP = re.compile(r'^\d{4}-\d\d-\d\d \d\d:\d\d:\d\d,\d{3}: ', flags=re.M)
CHATTER = re.compile(r'^(DEBUG|INFO) \[ann3depth\] .*\n', flags=re.M)
USAGE = re.compile(r'\Ausage: .*?^(?=\S+: error: )', flags=re.M | re.S)


def run(driver, argv):
    """(exit code, stdout, stderr) of one driver's main(argv) in this process, an argparse refusal included."""
    from ann3depth_amd import ann3depth, evaluate
    main = {'ann3depth': ann3depth.main, 'evaluate': evaluate.main}[driver]
    argv0, sys.argv[0] = sys.argv[0], driver + '.py'                       # argparse names the program in its error line
    out, err = io.StringIO(), io.StringIO()
    try:
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            try:
                code = main(list(argv))
            except SystemExit as e:
                code = e.code
    finally:
        sys.argv[0] = argv0
    return code, CHATTER.sub('', STAMP.sub('', out.getvalue())), USAGE.sub('', err.getvalue())


@pytest.mark.parametrize('case', CASES, ids=[c['driver'] + ' ' + ' '.join(c['argv']) for c in CASES])
def test_refusal_is_the_recorded_one(case):
    code, out, err = run(case['driver'], case['argv'])
    assert code == case['exit'] == 2
    assert out == case['stdout']
    assert err == case['stderr']
