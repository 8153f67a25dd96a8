# plain-C caller of the cube map entry points (no HIP headers, no C++): gcc + dlopen.  make -C tests/c -f cubemap_smoke.mk
cubemap_smoke: cubemap_smoke.c ../../include/swr.h
	gcc -O1 -std=c11 -Wall -Wextra -I../../include cubemap_smoke.c -o $@ -ldl
