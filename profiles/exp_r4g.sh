mkdir -p out
python -m pytest tests/test_gpu_parity.py tests/test_gpu_edge_cases.py -x -q -m gpu -k "halfline or sphere or c5 or spheres or nested" > out/r4g_tests.log 2>&1; tail -3 out/r4g_tests.log
python bench.py --full --steps 6 --warmup 2 --scene scenes/spheres64.txt --res 4096 4096 --depth 8 --batch 8 --cpu-spp 0 --per-iteration-sample 0 --repeats 5 2>out/r4g.err | python profiles/line_fields.py "c5 batch 8"
