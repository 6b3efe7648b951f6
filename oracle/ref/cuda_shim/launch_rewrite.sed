# kernel<<<grid, block[, shmem[, stream]]>>>(  ->  cuda_shim::launch("kernel", cuda_shim::cfg(...), <generic call>)(
# The one expression of a CUDA source that is not C++ (also written `<< <` ... `>> >`); nothing else changes.  The
# kernel's name may carry explicit template arguments.  Every rewritten site holds the marker cuda_shim::launch( once,
# which the recipes count.
s/([A-Za-z_][A-Za-z_0-9]*(<[^<>();]*>)?)[ \t]*<<[ \t]*<([^<>]*)>[ \t]*>[ \t]*>[ \t]*\(/cuda_shim::launch("\1", cuda_shim::cfg(\3), [](auto... a_){ \1(a_...); })(/g
