#!/usr/bin/env python3
"""Record tests/golden/plan_totals.json: for every case of tests/plan_cases.py the planner's totals of one
refine_alignment batch on the GPU (band cells, wave steps, reads redone by the exact kernel, tie flags).

Run it at the commit whose planner is the yardstick — tests/test_gpu_plan_shapes.py then holds later planners to the
same totals.  Usage: tools/record_plan_totals.py [OUT.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    import plan_cases
    from nadavca_amd import dtw
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'plan_totals.json')
    models, totals = {}, {}
    for case in plan_cases.build_cases():
        if case['model'] not in models:
            models[case['model']] = dtw.KmerModel(*plan_cases.model_arrays(case['model']))
        _, status, totals[case['name']] = plan_cases.run_case(dtw, case, models[case['model']])
        print('%-40s status %s %s' % (case['name'], status.tolist()[:6],
                                      {k: v for k, v in totals[case['name']].items() if k != 'tie_flags'}))
    with open(out, 'w') as f:
        json.dump(totals, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote %s (%d cases)' % (out, len(totals)))


if __name__ == '__main__':
    main()
