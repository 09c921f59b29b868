mkdir -p out/r4a
for b in 32 64 128; do for p in 1 2; do python bench.py --full --steps 20 --warmup 5 --repeats 7 --cpu-spp 0 --batch $b --pipeline $p 2>out/r4a/err_${b}_$p.txt | python profiles/line_fields.py "batch $b pipeline $p"; done; done > out/r4a/batch.txt 2>&1
cat out/r4a/batch.txt
