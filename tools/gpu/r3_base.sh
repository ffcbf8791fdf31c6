O=${AVEC_OUT:-$PWD/out}; mkdir -p $O
cd $GRAFT_REPO_ROOT
python bench.py --full --steps 30 --warmup 8 --no-cpu-baseline > $O/r3_base.json 2> $O/r3_base.err
timeout 600 python tools/find_copies.py > $O/r3_copies.log 2>&1
tail -3 $O/r3_base.err
head -c 3000 $O/r3_base.json
