for k in 0 2 4; do
  echo "== SRAD_WGRAD_KSPLIT=$k"
  if [ $k != 0 ]; then export SRAD_WGRAD_KSPLIT=$k; fi
  bash "$(dirname "$0")/wgrad_trace.sh"
done
