# plain-C caller of the mip chain entry points (no HIP headers, no C++): gcc + dlopen.  make -C tests/c -f mipmap_smoke.mk
mipmap_smoke: mipmap_smoke.c ../../include/swr.h
	gcc -O1 -std=c11 -Wall -Wextra -I../../include mipmap_smoke.c -o $@ -ldl
