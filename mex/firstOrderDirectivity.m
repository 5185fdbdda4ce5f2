function c = firstOrderDirectivity(a)
% The [1 x 4] real-SH coefficients of the first-order pattern a + (1 - a) * cos(gamma) about the source's front axis (host only;
% DESIGN.md section 15): c(1) = a * sqrt(4*pi), c(4) = (1 - a) * sqrt(4*pi/3) (the x term, n = 1, m = +1), the others 0.  a = 1 is
% omnidirectional, a = 0.5 a cardioid, a = 0 a figure of eight: the 'directivity' of getArrayIrs and getArrayRoomIrs.
c = [a * sqrt(4 * pi), 0, 0, (1 - a) * sqrt(4 * pi / 3)];
end
