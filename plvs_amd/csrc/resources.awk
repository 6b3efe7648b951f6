# `make resources`: the compiler's kernel-resource-usage remarks -> one line per kernel
#   <mangled name> VGPRs=.. AGPRs=.. ScratchSize=.. Occupancy=.. SGPRs_Spill=.. VGPRs_Spill=.. LDS_Size=..
# (ScratchSize in bytes per lane, Occupancy in waves per SIMD, LDS_Size in bytes per workgroup; the Makefile demangles)
function field(s) {
  sub(/.*remark: +/, "", s)
  sub(/ \[-Rpass.*/, "", s)
  sub(/ \[[a-zA-Z\/]+\]/, "", s)
  sub(/: /, "=", s)
  gsub(/ /, "_", s)
  return s
}
/remark: Function Name:/ {
  if (line != "") print line
  line = $0
  sub(/.*Function Name: /, "", line)
  sub(/ \[-Rpass.*/, "", line)
}
/remark: +(VGPRs|AGPRs|ScratchSize|Occupancy|SGPRs Spill|VGPRs Spill|LDS Size)/ { line = line " " field($0) }
END { if (line != "") print line }
